"""Inputs of the .bz2 writer's tests (test_bz2enc_host.py on the CPU, test_gpu_bz2enc.py on the GPU): no asserts about the
library here.  Built for level 1, where a block takes PIECE = 79 872 bytes of input, so that every case is tens to a few
hundred KiB; cases() gives (name, data) pairs, big_cases() the few that need a level above 1 to be one block, edge_cases()
the inputs chosen for how the kernels cut the work (tiles, lanes, groups a lane, bit offsets, buffer ends), a call of
snaphash_bzenc_stages_device each."""
import collections
import functools
import random

import xz_cases as X


def piece(level):
    """bzenc_piece: input bytes of a block."""
    return (100000 * level - 19) * 4 // 5 // 512 * 512


PIECE = piece(1)
assert PIECE == 79872 and piece(9) == 719872


def runs_of_four(n):
    """Runs of exactly four of alternating bytes: RLE1 makes five of every four."""
    return (b"aaaabbbb" * (n // 8 + 1))[:n]


def all_bytes(n, seed=11):
    r = random.Random(seed)
    return bytes(range(256)) + bytes(r.randrange(256) for _ in range(n - 256))


def one_row(n, row=5, seed=12):
    """Byte values of one 16-value row of the symbol map only (no byte twice in a row: RLE1 adds no count byte)."""
    r = random.Random(seed)
    out, last = bytearray(), 0
    for _ in range(n):
        last = (last + 1 + r.randrange(15)) % 16
        out.append(row * 16 + last)
    return bytes(out)


def sorted_runs(seed=13):
    """Long runs in the BWT's last column: ab x m has the last column b^m a^m, a zero run of m - 1."""
    out = []
    for k in range(1, 16):  # (2^16 needs more than a level-1 piece: big_cases)
        for d in (-1, 0, 1):
            out.append(("zero_run_2^%d%+d" % (k, d), b"ab" * ((1 << k) + d + 1)))
    return out


def sources_like(n, seed=15):
    """Program text: indented lines of a few identifiers, keywords and punctuation, blocks that open and close.  (xz_cases
    has generators for prose-like text, random bytes and random bytes with copies, none for sources.)"""
    r = random.Random(seed)
    idents = ["ctx", "slot", "n_blocks", "offset", "len", "rc", "out", "in_buf", "crc", "i", "k", "state", "hdr", "next_event"]
    types = ["uint32_t", "uint64_t", "const uint8_t*", "int", "size_t", "bool"]
    out, depth = bytearray(), 0
    while len(out) < n:
        ind = b"    " * depth
        k = r.randrange(10)
        if k < 3:
            out += ind + ("%s %s = %s + %d;\n" % (r.choice(types), r.choice(idents), r.choice(idents), r.randrange(64))).encode()
        elif k < 5:
            out += ind + ("if (%s %s %s) {\n" % (r.choice(idents), r.choice(["<", ">=", "==", "!="]), r.choice(idents))).encode()
            depth += 1
        elif k < 6:
            out += ind + ("for (%s %s = 0; %s < %s; ++%s) {\n" % ((r.choice(types),) + (r.choice(idents),) * 2 + (r.choice(idents),) + (r.choice(idents),))).encode()
            depth += 1
        elif k < 8 and depth:
            depth -= 1
            out += b"    " * depth + b"}\n"
        elif k < 9:
            out += ind + ("%s = %s(%s, %s);  // %s\n" % (r.choice(idents), r.choice(["fill", "launch", "reserve", "emit"]), r.choice(idents), r.choice(idents),
                                                        r.choice(X.WORDS))).encode()
        else:
            out += ind + ("return %s;\n" % r.choice(idents)).encode()
        depth = min(depth, 6)
    return bytes(out[:n])


def fibonacci(nsym=26, seed=14):
    """Byte value i occurs fib(i) times, shuffled: a Huffman code without a limit would be nsym - 1 bits deep."""
    r = random.Random(seed)
    a, b, vals = 1, 1, []
    for i in range(nsym):
        vals += [i] * a
        a, b = b, a + b
    r.shuffle(vals)
    return bytes(vals)


@functools.lru_cache(maxsize=None)
def cases():
    P = PIECE
    c = []
    for n in (0, 1, 2, 3, 4, 5, P - 1, P, P + 1, 2 * P, 2 * P + 1):
        c.append(("text_%d" % n, X.text(n, seed=20 + n % 7) if n else b""))
    c.append(("one_byte_3", b"zzz"))                       # one distinct byte: 3 symbols, two tables, one selector
    c.append(("one_byte_piece", b"\x00" * P))             # periodic after RLE1 (four zeros and a count of 255, over and over)
    c.append(("one_byte_1000", b"z" * 1000))
    c.append(("ab_x_1000", b"ab" * 1000))                  # periodic: 1000 ties at origPtr
    c.append(("abc_x_700", b"abc" * 700))
    c.append(("ab_piece_and_a_half", b"ab" * (P * 3 // 4)))
    c.append(("runs_of_four_piece", runs_of_four(P)))     # RLE1 gives P * 5 / 4 = 99 840: the cap at its edge
    c.append(("runs_of_four_two_pieces", runs_of_four(2 * P)))
    for n in (255, 258, 259, 260, 263, 518):
        c.append(("run_%d" % n, b"x" + b"r" * n + b"y"))
        c.append(("run_%d_alone" % n, b"r" * n))
    for k in range(0, 6):  # a run across a piece boundary at every split of its first five bytes
        c.append(("run_across_%d" % k, X.text(P - k, seed=31) + b"\x07" * 300 + X.text(100, seed=32)))
    c.append(("all_256_values", all_bytes(20000)))
    c.append(("one_map_row", one_row(5000)))
    c.extend(sorted_runs())
    c.append(("random32k_repeated", (X.rnd(32768, seed=41) * 3)[:P]))  # doubling runs to its last rounds
    c.append(("text_300k", X.text(300000, seed=42)))
    c.append(("sources_like_200k", sources_like(200000)))
    c.append(("sprinkled", X.sprinkled(300, 40, seed=43, times=3000)))  # random bytes with short copies
    c.append(("random_100k", X.rnd(100000, seed=44)))
    c.append(("six_pieces", X.text(5 * P + 1234, seed=45)))
    return c


@functools.lru_cache(maxsize=None)
def big_cases():
    """(name, data, level): one block only above level 1."""
    return [
        ("zero_run_2^16-1", b"ab" * (1 << 16), 9),
        ("zero_run_2^16", b"ab" * ((1 << 16) + 1), 9),
        ("zero_run_2^16+1", b"ab" * ((1 << 16) + 2), 9),
        ("fibonacci", fibonacci(), 9),
    ]


NMTF_LIMITS = (199, 200, 599, 600, 1199, 1200, 2399, 2400)


def nmtf_cases(nmtf_of):
    """Inputs whose one block has exactly the MTF symbol counts at which the table count changes, found with the host model
    (nmtf_of(data) -> nMTF): random bytes, a symbol a byte but for the zero runs."""
    out = []
    for target in NMTF_LIMITS:
        for n in range(max(1, target - 120), target + 2):
            d = X.rnd(n, seed=1000 + target)
            if nmtf_of(d) == target:
                out.append(("nmtf_%d" % target, d))
                break
        else:
            raise AssertionError("no input with nMTF %d" % target)
    return out


# ---- the kernels' own edges (test_bz2enc_host.py ties them to the model, test_gpu_bz2enc_edges.py runs them) ----
# One Edge is one call of snaphash_bzenc_stages_device.  kind "pieces": `ranges` (offset, length) of `data`; "last": the
# from_last mode, `columns` of (last column, origPtr, CRC); "guard": ranges of which exactly one has more RLE1 output than
# `cap`.  cap 0: the producer's.
Edge = collections.namedtuple("Edge", "name kind level cap carry carry_bits data ranges columns")

TILE = 1024          # lanes of the RLE1 kernel: source bytes a sweep
RUN_LENS = (4, 5, 258, 259, 260, 263)
RUN_OFFS = (0, 1019, 1020, 1021, 1022, 1023, 1024)
MTF_POSITIONS = (1, 2, 3, 4, 5, 7, 8, 63, 64, 127, 128, 251, 252, 253, 254, 255)
FRONT_RUNS = sorted({1, 2, 3, 63, 64, 65} | {(1 << k) + d for k in range(1, 11) for d in (-1, 0, 1)})
FRONT_RUN_OFFS = (60, 61, 62, 63, 64)
GROUP_COUNTS_L1 = (1, 2, 1023, 1024, 1025)
GROUP_COUNTS_L2 = (2047, 2048, 2049)   # (a level-1 piece of random bytes has 1598 groups at most)
LAST_GROUPS = (1, 49, 50)
GUARD_CAP = 1024
CONCAT_BLOCKS = 320


def no_runs(n, seed, row=5):
    """n bytes of 16 values, none equal to its left neighbour: RLE1 copies them."""
    return one_row(n, row, seed)


def _ranges(parts):
    """parts: (bytes before the range, the range's bytes, bytes behind it) -> (data, ranges)"""
    data, ranges = bytearray(), []
    for before, body, behind in parts:
        data += before
        ranges.append((len(data), len(body)))
        data += body + behind
    return bytes(data), ranges


def rle1_tile_edges():
    parts, what = [], []
    for L in RUN_LENS:            # the first four bytes, the count and the lookahead across a tile's end
        for off in RUN_OFFS:
            parts.append((b"", no_runs(off, 100 + off) + b"\xee" * L + no_runs(300, 200 + L), b""))
            what.append(("run", L, off))
    # a run that began two tiles back: its groups of 259 go on through two tile ends
    parts.append((b"", no_runs(100, 7) + b"\xee" * (2 * TILE + 300) + no_runs(50, 8), b""))
    what.append(("long_run", 2 * TILE + 300, 100))
    for k in (3, 4, 5):           # the range ends k bytes into a run that the buffer continues
        parts.append((b"", no_runs(1500, 300 + k) + b"\xee" * k, b"\xee" * 300))
        what.append(("cut_run", k, 1500))
    for n in (1, 2, 1023, 1024, 1025):
        parts.append((b"\x00", X.text(n, seed=400 + n), b"\x00"))
        what.append(("len", n, 0))
    data, ranges = _ranges(parts)
    return Edge("rle1_tile_edges", "pieces", 1, 4096, 0, 0, data, ranges, None), what


def fours_of_different_bytes(n, seed):
    """Runs of exactly four, each of another byte than the last: RLE1 makes five of every four."""
    r = random.Random(seed)
    vals, last = bytearray(), 0
    for _ in range(n // 4):
        last = (last + 1 + r.randrange(255)) % 256
        vals.append(last)
    return bytes(b for v in vals for b in (v, v, v, v))


def mtf_walk(positions, alphabet):
    """The last column a decoder gets from these move-to-front positions over `alphabet` (sorted byte values)."""
    lst, out = list(alphabet), bytearray()
    for p in positions:
        v = lst.pop(p)
        lst.insert(0, v)
        out.append(v)
    return bytes(out)


def mtf_edges():
    cols, what = [], []
    for p in MTF_POSITIONS:       # always the byte at list position p: every symbol is p + 1, p + 1 bytes used
        cols.append(mtf_walk([p] * 700, range(256)))
        what.append(("position", p))
    r = random.Random(51)
    sparse = sorted(r.sample(range(256), 200))  # seq[] is not the byte value
    cols.append(mtf_walk([r.randrange(200) for _ in range(900)], sparse))
    what.append(("sparse", 200))
    cols.append(mtf_walk([r.choice((0, 0, 1, 2, 3, 4, 199)) for _ in range(900)], sparse))
    what.append(("sparse", 200))
    for n in (1, 63, 64, 65):
        cols.append(mtf_walk([r.randrange(1, 40) for _ in range(n)], range(100, 140)))
        what.append(("n", n))
    cols.append(b"q" * 500)       # one byte only: a front run and the end-of-block symbol
    what.append(("one_byte", 500))
    columns = [(c, (7 * k + len(c) // 2) % len(c), 0x9e3779b9 * (k + 1) & 0xffffffff) for k, c in enumerate(cols)]
    return Edge("mtf_positions", "last", 1, 1024, 0, 0, None, None, columns), what


def front_run_edges():
    cols, what = [], []
    for R in FRONT_RUNS:          # a run of R front bytes that begins at offset off of a 64-symbol tile and ends the block
        for off in FRONT_RUN_OFFS:
            pre = bytes(b"abc"[i % 3] for i in range(64 + off - 1)) + b"x"
            cols.append(pre + b"x" * R)
            what.append((R, 64 + off))
    columns = [(c, k % len(c), 0x01000193 * (k + 1) & 0xffffffff) for k, c in enumerate(cols)]
    return Edge("front_runs", "last", 1, 1280, 0xc0, 2, None, None, columns), what


def _random_with(nmtf_of, level, want, n0, seed):
    """The shortest X.rnd(n, seed), n >= n0, whose block has an nMTF that `want` accepts."""
    for n in range(max(1, n0), n0 + 400):
        d = X.rnd(n, seed=seed)
        if want(nmtf_of(d, level)):
            return d
    raise AssertionError("no random input from %d bytes on with the nMTF asked for" % n0)


def coding_edges(nmtf_of):
    """nmtf_of(data, level) -> the nMTF of the one block: the host model's."""
    out = []
    for level, counts in ((1, GROUP_COUNTS_L1), (2, GROUP_COUNTS_L2)):
        parts = []
        for ng in counts:         # `per` of the coding kernel is ceil(ng / 1024)
            parts.append(_random_with(nmtf_of, level, lambda m, ng=ng: (m + 49) // 50 == ng, 50 * (ng - 1) - 30, 2000 + ng))
        if level == 1:
            for lg in LAST_GROUPS:  # symbols of the last group
                parts.append(_random_with(nmtf_of, level, lambda m, lg=lg: (m - 1) % 50 + 1 == lg, 3000 + lg, 2100 + lg))
        data, ranges = _ranges([(b"", p, b"") for p in parts])
        out.append(Edge("group_counts_level%d" % level, "pieces", level, 0, 0, 0, data, ranges, None))
    return out


def most_groups_column(seed=61):
    """899 840 bytes, none equal to its left neighbour (every MTF position >= 1: nMTF = n + 1, 17 997 groups), the
    positions 1..25 drawn with Fibonacci weights: a Huffman code without a limit would be 24 bits deep."""
    r = random.Random(seed)
    n = piece(9) // 4 * 5
    w, a, b = [], 1, 1
    for _ in range(25):
        w.append(a)
        a, b = b, a + b
    return mtf_walk(r.choices(range(1, 26), weights=w, k=n), range(0, 52, 2))


def concat_edges():
    r = random.Random(71)
    parts = [(b"", X.text(1 + (k * 37 + r.randrange(200)) % 200, seed=500 + k), b"") for k in range(CONCAT_BLOCKS)]
    data, ranges = _ranges(parts)
    return [Edge("concat_%d_blocks_carry_%d" % (CONCAT_BLOCKS, cb), "pieces", 1, 1024, carry, cb, data, ranges, None)
            for cb, carry in ((0, 0), (1, 0x80), (7, 0xaa))]


GUARD_OUTPUTS = (GUARD_CAP + 1, GUARD_CAP + 64, GUARD_CAP + 65, GUARD_CAP + 64 + 1000)


def guard_edges():
    """cap 1024.  accepted: RLE1 output of exactly cap.  Then one range with more, last in the launch and in the middle of
    it (behind it a range of one byte: whatever a store past the stride hits there must keep the fill).  An unguarded
    store lands at most 1000 bytes behind the block's cap + 64."""
    small = [X.text(n, seed=600 + n) for n in (150, 1, 90)]
    big = {n: no_runs(n, 700 + n) for n in (GUARD_CAP,) + GUARD_OUTPUTS}
    # a fourth byte and its count across the room's end: 1084 bytes, then a run of four -- the pair would end at 1089
    big["straddle"] = no_runs(GUARD_CAP + 60, 777) + b"\xee" * 4 + no_runs(200, 778)
    out = []
    data, ranges = _ranges([(b"", small[0], b""), (b"", big[GUARD_CAP], b""), (b"", small[1], b""), (b"", small[2], b""), (b"", big[GUARD_CAP], b"")])
    out.append(Edge("guard_exactly_cap", "pieces", 1, GUARD_CAP, 0, 0, data, ranges, None))
    for key in GUARD_OUTPUTS + ("straddle",):
        data, ranges = _ranges([(b"", small[0], b""), (b"", small[2], b""), (b"", big[key], b"")])
        out.append(Edge("guard_%s_last" % key, "guard", 1, GUARD_CAP, 0, 0, data, ranges, None))
        data, ranges = _ranges([(b"", small[0], b""), (b"", big[key], b""), (b"", small[1], b""), (b"", small[2], b"")])
        out.append(Edge("guard_%s_middle" % key, "guard", 1, GUARD_CAP, 0, 0, data, ranges, None))
    return out


def edge_names():
    """edge_cases()' names, without the model (a test's parameters)"""
    n = ["rle1_tile_edges", "fours_full_piece_level1", "fours_full_piece_level9", "mtf_positions", "front_runs", "group_counts_level1",
         "group_counts_level2", "most_groups_level9", "fibonacci_level9"]
    n += ["concat_%d_blocks_carry_%d" % (CONCAT_BLOCKS, cb) for cb in (0, 1, 7)] + ["guard_exactly_cap"]
    return n + ["guard_%s_%s" % (k, w) for k in GUARD_OUTPUTS + ("straddle",) for w in ("last", "middle")]


@functools.lru_cache(maxsize=None)
def edge_cases(nmtf_of):
    """Every Edge, by name order of the stages.  nmtf_of(data, level): the host model's nMTF of a one-block input."""
    e = [rle1_tile_edges()[0]]
    for level in (1, 9):
        d = fours_of_different_bytes(piece(level), 80 + level)
        e.append(Edge("fours_full_piece_level%d" % level, "pieces", level, 0, 0, 0, d, [(0, len(d))], None))
    e += [mtf_edges()[0], front_run_edges()[0]]
    e += coding_edges(nmtf_of)
    col = most_groups_column()
    e.append(Edge("most_groups_level9", "last", 9, 0, 0, 0, None, None, [(col, len(col) // 3, 0xdeadbeef)]))
    fib = fibonacci()
    e.append(Edge("fibonacci_level9", "pieces", 9, 0, 0xe0, 3, fib, [(0, len(fib))], None))
    e += concat_edges()
    e += guard_edges()
    return e
