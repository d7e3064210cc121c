"""Inputs for the .xz writer's tests (test_xzenc_host.py on the CPU, test_gpu_xzenc.py on the GPU): (name, bytes, block
size) triples, each the smallest at which the thing it is named for can go wrong.  No asserts about the library here.

The Block size is 128 KiB -- the smallest with two LZMA2 chunks of 65 536 bytes -- unless the case is about the Block
size.  No input is larger than three Blocks, but for the one Block of the default size and the one of 4 MiB, the largest
a Block may be (far_dists: generated, 4 MiB of mostly zero bytes).

The inputs from tails_3 on are about the encoder's kernels stage by stage (test_gpu_xzenc_edges.py holds the arrays the
kernels leave in HBM against the model's; test_xzenc_host.py shows that each shape occurs)."""
import functools
import random

import xz_cases as X

KiB = 1024
CHUNK = 65536
B = 128 * KiB

DIST_EDGES_SMALL = (1, 2, 3, 4, 5, 127, 128, 129)
DIST_EDGES_FAR = (65535, 65536, 65537, 131000)
PERIODS = (1, 2, 63, 64, 65, 273)
BOUNDARY_PATTERN = 3000
NONE = 0xFFFFFFFF
TILE = 64                                     # positions the chains kernel links at a time
TAILS = (3, 4, 5, 63, 64, 65)                 # last Blocks around "four bytes to hash" and around a tile
GROUP_PERIODS = (3, 4, 5, 7, 16, 31, 32, 33)  # distinct hashes in a tile of that period
GROUP_FILLERS = (1, 7, 31, 33, 63)            # random bytes in front of a period, walked through in turn
GROUP_RUN = 300                               # bytes of a period (no multiple of the tile: every start is aligned differently)
FAR_BLOCK = 4 << 20
FAR_DISTS = tuple(d for k in range(17, 22) for d in ((1 << k) - 1, 1 << k, (1 << k) + 1))
FAR_MAX = FAR_BLOCK - 273                     # the farthest match of full length in a Block: 4 194 031
# rnd(k) + text(65536 - k) in one chunk, at the line 6 + csize < 3 + usize (csize <= 65 532).  Found by scanning k with
# the host model (tests/test_xzenc_host.py asserts both verdicts and how near the line the first one is):
MARGIN_LZMA_K = 64048     # the largest k still written as LZMA: the model's csize is 65 531
MARGIN_STORED_K = 64049   # stored, as is every k above it: by the verdict after the flush, every byte coded
MARGIN_GIVEUP_K = 64061   # the smallest k at which the coder gives up inside its loop: 65 531 of the 65 536 bytes coded
# text(65536) + t zero bytes in one Block: the tail chunk of t bytes is LZMA from this t on (6 + csize < 3 + t with
# csize >= 5 needs t >= 9; the model's csize is 7, so 13 < 14 at t = 11 and not 13 < 13 at t = 10), stored below it
TAIL_MIN_T = 11


def dist_edges():
    """A 4 KiB random pattern at Block offset 100 and again 65 535, 65 536, 65 537 and 131 000 bytes behind the copy in
    front of it (into an earlier chunk of the same Block: the nearest occurrence is always the previous copy), random
    filler between the copies; then short periods of 1 .. 129 bytes: the distance slots' edges and the reverse trees'
    limit."""
    r = random.Random(77)
    pat = r.randbytes(4096)
    out = bytearray(r.randbytes(100)) + pat
    at = 100
    for d in DIST_EDGES_FAR:
        out += r.randbytes(at + d - len(out))
        at += d
        out += pat
    for d in DIST_EDGES_SMALL:
        out += r.randbytes(9) + X.periodic(d, 300, seed=5)
    return bytes(out)


def boundary(block=B):
    """The same random pattern at the end of Block 0 and at the start of Block 1."""
    pat = X.rnd(BOUNDARY_PATTERN, 91)
    return X.text(block - BOUNDARY_PATTERN, 92) + pat + pat + X.text(5000, 93)


def hash32(four):
    """xz_enc_core.h's xzenc_hash of a 4-byte value loaded little-endian (test_xzenc_host.py holds it against the header's)."""
    return ((four * 2654435761) & 0xFFFFFFFF) >> 17


def tail_bytes(k):
    """k bytes whose last hashable position (k - 4) repeats the first one's four bytes: it has an earlier position to link to."""
    if k < 8:
        return b"z" * k
    t = X.text(k, 100 + k)
    return t[:k - 4] + t[:4]


def tile_groups():
    """(bytes, where each period's run starts)."""
    r = random.Random(78)
    out, starts = bytearray(), []
    for i, p in enumerate(GROUP_PERIODS):
        out += r.randbytes(GROUP_FILLERS[i % len(GROUP_FILLERS)])
        starts.append(len(out))
        out += X.periodic(p, GROUP_RUN - p, seed=6)
    out += r.randbytes(9)
    assert len({s % TILE for s in starts}) == len(starts)
    return bytes(out), starts


@functools.lru_cache(maxsize=None)
def twin_values():
    """Two 4-byte strings with different first bytes and the same hash."""
    r = random.Random(79)
    seen = {}
    while True:
        v = r.randbytes(4)
        w = seen.setdefault(hash32(int.from_bytes(v, "little")), v)
        if w[0] != v[0]:
            return w, v


TWIN_AT = (64 * 3 + 10, 64 * 3 + 18, 64 * 7 + 60, 64 * 8 + 4)  # a, b in one tile, 8 bytes apart; a, b again in adjacent tiles


def hash_twins():
    a, b = twin_values()
    out = bytearray(random.Random(80).randbytes(64 * 10))
    for at, v in zip(TWIN_AT, (a, b, a, b)):
        out[at:at + 4] = v
    return bytes(out)


def far_dists():
    """(bytes, [(first copy, distance)])."""
    r = random.Random(81)
    out = bytearray(FAR_BLOCK)
    used, where = [], []

    def put(at, pat):
        assert all(at + len(pat) <= a or b <= at for a, b in used) and at + len(pat) <= FAR_BLOCK
        used.append((at, at + len(pat)))
        out[at:at + len(pat)] = pat

    pat = bytes(r.randrange(1, 256) for _ in range(273))
    put(0, pat)
    put(FAR_MAX, pat)
    for i, d in enumerate(FAR_DISTS):
        pat = bytes(r.randrange(1, 256) for _ in range(64))
        put(1024 * (i + 1), pat)
        put(1024 * (i + 1) + d, pat)
        where.append((1024 * (i + 1), d))
    return bytes(out), where


def margin(k):
    return X.rnd(k, 94) + X.text(CHUNK - k, 95)


def tail_min(t):
    return X.text(CHUNK, 96) + bytes(t)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for n in (0, 1, 2, 65535, 65536, 65537, 131071, 131072, 131073, 3 * B + 1):
        out.append(("len_%d" % n, X.text(n, 50 + n % 7), B))
    out.append(("block_64k", X.text(2 * CHUNK + 5, 60), CHUNK))
    out.append(("block_default", X.text((1 << 20) + 100, 61), 0))
    out.append(("block_4m", X.text(70000, 62), 4 << 20))
    out.append(("incompressible", X.rnd(2 * B, 63), B))
    out.append(("mixed_rtrt", X.rnd(CHUNK, 64) + X.text(CHUNK, 65) + X.rnd(CHUNK, 66) + X.text(CHUNK, 67), 256 * KiB))
    out.append(("mixed_tr", X.text(CHUNK, 68) + X.rnd(CHUNK, 69), B))
    for p in PERIODS:
        out.append(("period_%d" % p, X.periodic(p, 70000 - p), B))
    out.append(("all_bytes_twice", bytes(range(256)) * 2, B))
    out.append(("dist_edges", dist_edges(), 512 * KiB))
    out.append(("sprinkled", X.sprinkled(64, 2) + X.sprinkled(1, 2), B))
    out.append(("boundary", boundary(), B))
    for k in TAILS:
        out.append(("tails_%d" % k, X.text(CHUNK, 97) + tail_bytes(k), CHUNK))
    out.append(("tile_groups", tile_groups()[0], B))
    out.append(("hash_twins", hash_twins(), B))
    out.append(("far_dists", far_dists()[0], FAR_BLOCK))
    out.append(("margin_lzma", margin(MARGIN_LZMA_K), B))
    out.append(("margin_stored", margin(MARGIN_STORED_K), B))
    out.append(("margin_giveup", margin(MARGIN_GIVEUP_K), B))
    out.append(("tail_min", tail_min(TAIL_MIN_T), B))
    out.append(("tail_min_less", tail_min(TAIL_MIN_T - 1), B))
    return out


def by_name(name):
    return next(c for c in cases() if c[0] == name)
