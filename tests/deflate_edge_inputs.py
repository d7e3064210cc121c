"""Whole inputs for the DEFLATE compressor's own geometry (snappy_amd/csrc/deflate_core.h): segments of kDfSeg = 1920
positions (30 tiles of 64), chunks of 65536, a window of kDfMaxDist = 28800 = 15 segments, matches of at most 258 bytes,
staging pieces whose first chunk has no window.  Shared by tests/test_f3_host.py (the CPU model must show, by its counters,
the shape each input is named for) and tests/test_gpu_deflate_edges.py (the kernel's bytes must equal the model's).

edge_inputs() -> {name: Case}.  Case.piece is the staging piece (Context(staging_bytes=...) and the model's `piece`),
Case.depth the search depth asked of the Context (0 = the default; the model runs at effective_depth(Case.depth)),
Case.want what the model's counters must show (check_shape below).
No input is longer than three chunks."""
import collections

import numpy as np

SEG, CHUNK, MAX_DIST, MAX_MATCH = 1920, 65536, 28800, 258
PIECE = 3 * CHUNK   # one staging piece holds every input whole: chunks after the first have their window
SEED = 1952

# the model's counters (tests/f3_host_harness.cpp: ModelCounters), in order
COUNTERS = ("chunks", "stored", "fixed", "dynamic", "matches", "longest_match", "farthest_dist", "window_matches", "dist0_chunks",
            "dist1_chunks", "ll_rounds", "d_rounds", "cl_rounds", "ll_depth", "d_depth", "cl_depth")
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)

Case = collections.namedtuple("Case", "data piece depth want")

SIZES = sorted({SEG - 1, SEG, SEG + 1} | {SEG * k + d for k in (2, 15, 34) for d in (-1, 1)} |
               {CHUNK + d for d in (1, 63, 64, 65, SEG - 1, SEG, SEG + 1)} | {MAX_DIST - 1, MAX_DIST, MAX_DIST + 1})


def _prose(rng, n):
    words = [bytes(rng.integers(97, 123, size=int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(400)]
    out = b" ".join(words[int(i)] for i in rng.integers(0, 400, size=n // 3 + 8))
    assert len(out) >= n
    return out[:n]


def _rand(rng, n):
    return rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()


def _repeat_at(rng, total, src, dist, length):
    """Random bytes with ONE planted repeat: `length` bytes at src again at src + dist, the bytes in front of and behind
    the two copies made to differ, so the repeat is neither longer nor does it start earlier."""
    buf = bytearray(_rand(rng, total))
    dst = src + dist
    assert src >= 1 and dst + length + 1 <= total
    buf[dst:dst + length] = buf[src:src + length]
    buf[dst - 1] = buf[src - 1] ^ 0xff
    buf[dst + length] = buf[src + length] ^ 0xff
    return bytes(buf)


def limiter_recipe(seed, shuffled):
    """The input that drives the code length code past 7 bits: 12 000 random bytes, then 12-byte copies from the base
    distances of distance codes 4 to 20, a Fibonacci number of copies per code (ascending by code, or all of them in
    shuffled order), two random bytes behind each, cut at a chunk.  The distance code's lengths come out as a ladder, and
    the run-length symbols of the header with them."""
    rng = np.random.default_rng(seed)
    buf = bytearray(_rand(rng, 12000))
    fibs, a, b = [], 1, 1
    for _ in range(4, 21):
        fibs.append(a)
        a, b = b, a + b
    plan = [code for code, cnt in zip(range(4, 21), fibs) for _ in range(cnt)]
    if shuffled:
        plan = [plan[i] for i in rng.permutation(len(plan))]
    for code in plan:
        if len(buf) >= CHUNK:
            break
        d = DIST_BASE[code]
        for _ in range(12):
            buf.append(buf[-d])
        buf += _rand(rng, 2)
    return bytes(buf[:CHUNK])


# seeds (and order) for which the model's counters show the 7-bit limiter firing; test_f3_host asserts that they still do
LIMITER_SEEDS = ((2, True), (8, False))


def effective_depth(depth):
    """What the library makes of snaphash_config.deflate_depth (include/snaphash.h: 0 = the default; otherwise 4 .. 256,
    rounded down to a multiple of 4 -- the kernel walks whole batches of four links): the depth the model must run at."""
    return 0 if depth == 0 else min(max(depth, 4), 256) & ~3


def edge_inputs():
    rng = np.random.default_rng(SEED)
    prose = _prose(rng, 3 * CHUNK)
    noise = _rand(rng, 3 * CHUNK)
    cases = {}
    for n in SIZES:
        nch = (n + CHUNK - 1) // CHUNK
        # compressible: the first chunk goes out with dynamic codes, a tail of a few bytes stored or fixed
        cases["prose %d" % n] = Case(prose[:n], PIECE, 0, {"chunks": nch, "dynamic>=": 1, "matches>=": 100})
        cases["random %d" % n] = Case(noise[:n], PIECE, 0, {"chunks": nch, "stored": nch})
    # ---- match geometry: one planted repeat of 40 bytes in random bytes ----
    far = {"longest_match": 40, "farthest_dist": MAX_DIST}
    cases["repeat at 28800 inside the first chunk"] = Case(_repeat_at(rng, 40000, 700, MAX_DIST, 40), PIECE, 0, dict(far, chunks=1, window_matches=0))
    cases["repeat at 28801 inside the first chunk"] = Case(_repeat_at(rng, 40000, 700, MAX_DIST + 1, 40), PIECE, 0, {"chunks": 1, "longest_match<": 40})
    across = _repeat_at(rng, CHUNK + 5000, CHUNK + 1000 - MAX_DIST, MAX_DIST, 40)  # the copy in the second chunk, its source in the first
    cases["repeat at 28800 from the previous chunk"] = Case(across, PIECE, 0, dict(far, chunks=2, **{"window_matches>=": 1}))
    cases["repeat at 28801 from the previous chunk"] = Case(_repeat_at(rng, CHUNK + 5000, CHUNK + 1000 - MAX_DIST - 1, MAX_DIST + 1, 40), PIECE, 0,
                                                            {"chunks": 2, "longest_match<": 40})
    # the same bytes with the second chunk first in its staging piece: no window, the repeat is not there to be found
    cases["repeat at 28800, the chunk first in its piece"] = Case(across, CHUNK, 0, {"chunks": 2, "window_matches": 0, "longest_match<": 40})
    for length in (257, 258, 259):
        cases["repeat of %d bytes" % length] = Case(_repeat_at(rng, 12000, 300, 5000, length), PIECE, 0,
                                                    {"chunks": 1, "longest_match": min(length, MAX_MATCH), "farthest_dist>=": 5000})
    # compressible, across chunks: matches reach back into the previous chunk; with one-chunk pieces none can
    cases["prose, three chunks of one piece"] = Case(prose[:2 * CHUNK + 777], PIECE, 0, {"chunks": 3, "window_matches>=": 100})
    cases["prose, every chunk a piece"] = Case(prose[:2 * CHUNK + 777], CHUNK, 0, {"chunks": 3, "window_matches": 0})
    # a chunk whose matches all have one distance symbol (the model completes the distance code with a second), and none at all
    cases["one byte 5000 times"] = Case(b"q" * 5000, PIECE, 0, {"chunks": 1, "dist1_chunks": 1, "farthest_dist": 1, "longest_match": MAX_MATCH})
    cases["no two bytes alike"] = Case(bytes(range(256)), PIECE, 0, {"chunks": 1, "dist0_chunks": 1, "matches": 0})
    # ---- the code length code's limiter through real input ----
    for seed, shuffled in LIMITER_SEEDS:
        cases["code length code limiter, seed %d%s" % (seed, " shuffled" if shuffled else "")] = Case(
            limiter_recipe(seed, shuffled), PIECE, 0, {"chunks": 1, "dynamic": 1, "cl_rounds>=": 2, "cl_depth>=": 8})
    # ---- the search depth at both ends ----
    for depth in (1, 128):
        cases["prose %d at depth %d" % (CHUNK + SEG + 1, depth)] = Case(prose[:CHUNK + SEG + 1], PIECE, depth, {"chunks": 2, "dynamic>=": 1})
        cases["repeat at 28800 from the previous chunk at depth %d" % depth] = Case(
            across, PIECE, depth, {"chunks": 2, "longest_match<": 40} if depth == 1 else dict(far, chunks=2))  # the four links a depth of 1 is raised to do not get there
    assert all(len(c.data) <= 3 * CHUNK for c in cases.values())
    return cases


def check_shape(name, want, got):
    """want: {"counter": exact, "counter>=": at least, "counter<": below}; got: {counter: value}."""
    for key, v in want.items():
        if key.endswith(">="):
            assert got[key[:-2]] >= v, (name, key, v, got)
        elif key.endswith("<"):
            assert got[key[:-1]] < v, (name, key, v, got)
        else:
            assert got[key] == v, (name, key, v, got)
