"""Inputs that reach ranges_equal_kernel (sha512_kernels.hip), launch_compare_ranges and the staged pass of
files_equal_impl (snaphash_api.cpp) at their own edges, and fill_synthetic_kernel at its two: plain numpy, no GPU, no
library, everything seeded.  tests/test_cmp_edges_host.py checks on the CPU that every case is what it claims (its
closed-form verdicts are the ones a plain byte compare gives); tests/test_gpu_cmp_edges.py sends the cases through the
kernels.

A case names the bytes of side A, and for every pair which A range it is compared with, and which bits of its own copy
of that range are flipped.  The verdict has a closed form: a pair is equal iff none of its flipped bytes lies below its
length.  materialise() lays the B side out: every range, on either side, is followed by at least SLACK bytes that differ
between the sides (0xA5 under A, 0x5A under B).  The kernel loads the 16-byte piece that holds a range's last byte whole:
the slack keeps that load inside the buffer, and a compare that forgot to mask the bytes past the end says "differ".

The groups, and what each one decides in the code:
  A  every 16-byte piece, at lengths around the bounds of the unrolled loop (p + 768 < nwhole, stride 1024), its
     hand-over to the stride-256 loop, and the verdict write of each wave (one lane of one wave sees the difference)
  B  a full chunk of 256 KiB, a chunk one piece short with a 3-byte tail, and a second chunk of one byte
  C  the tail mask: every count of valid bytes 1..15, a flip in every byte of the last piece, low and high bit
  D  chunk tables: pairs of several chunks between pairs of none, ch.pair against the verdict byte, in two orders
  E  200 000 pairs of 0..80 bytes
  F  both sides in one allocation, a range against itself, two bases with different offsets throughout"""
import numpy as np

PIECE = 16
CHUNK = 256 << 10  # sha512_kernels.h kCmpChunk
SLACK = 64
FILL_A, FILL_B = 0xA5, 0x5A


def pad16(n):
    return (n + 15) // 16 * 16


def ranges_equal_ref(a, off_a, b, off_b, lens):
    """The reference: exactly lens[i] bytes of each side, nothing else."""
    out = np.empty(len(lens), dtype=np.uint8)
    for i in range(len(lens)):
        oa, ob, n = int(off_a[i]), int(off_b[i]), int(lens[i])
        out[i] = np.array_equal(a[oa:oa + n], b[ob:ob + n])
    return out


def _starts(sizes):
    out = np.zeros(len(sizes), dtype=np.int64)
    np.cumsum(sizes[:-1], out=out[1:])
    return out


def make_case(name, a_len, a_data, src, flip_pair, flip_pos, flip_mask, tag, lead=0, **meta):
    """a_len: the lengths of the A ranges, a_data: their bytes end to end; src[i]: the A range of pair i; flip_*: one
    entry per flipped bit (pair, byte position in the pair's copy, mask); tag[i]: what report() shows for pair i (a
    piece or byte index, -1: nothing flipped); lead: bytes in front of the first A range."""
    a_len = np.asarray(a_len, dtype=np.int64)
    src = np.asarray(src, dtype=np.int64)
    a_off = lead + _starts(pad16(a_len) + SLACK)
    a = np.full(lead + int((pad16(a_len) + SLACK).sum()), FILL_A, dtype=np.uint8)
    a[np.repeat(a_off - _starts(a_len), a_len) + np.arange(int(a_len.sum()))] = a_data
    fp, fo, fm = (np.asarray(x, dtype=t) for x, t in ((flip_pair, np.int64), (flip_pos, np.int64), (flip_mask, np.uint8)))
    lens = a_len[src]
    assert np.all(fm != 0) and np.all(fo < pad16(lens[fp]) + SLACK) and len(set(zip(fp.tolist(), fo.tolist()))) == len(fp)
    expected = np.ones(len(src), dtype=np.uint8)
    expected[fp[fo < lens[fp]]] = 0  # the closed form
    return dict(name=name, a=a, a_off=a_off, a_len=a_len, src=src, lens=lens, flip_pair=fp, flip_pos=fo, flip_mask=fm,
                tag=np.asarray(tag, dtype=np.int64), expected=expected, **meta)


def materialise(case):
    """-> the layout of a call: a, off_a, b, off_b, lens (offsets and lengths as the uint64 arrays the ABI takes)."""
    a, src, lens = case["a"], case["src"], case["lens"]
    stride = pad16(lens) + SLACK
    off_b = _starts(stride)
    b = np.full(int(stride.sum()), FILL_B, dtype=np.uint8)
    cuts = np.concatenate(([0], np.flatnonzero(src[1:] != src[:-1]) + 1, [len(src)]))
    for s, e in zip(cuts[:-1].tolist(), cuts[1:].tolist()):  # a run of pairs that copy the same A range
        n, st, oa, ob = int(lens[s]), int(stride[s]), int(case["a_off"][src[s]]), int(off_b[s])
        if n:
            b[ob:ob + (e - s) * st].reshape(e - s, st)[:, :n] = a[oa:oa + n]
    b[off_b[case["flip_pair"]] + case["flip_pos"]] ^= case["flip_mask"]
    u = lambda x: np.ascontiguousarray(x, dtype=np.uint64)
    return dict(a=a, off_a=u(case["a_off"][src]), b=b, off_b=u(off_b), lens=u(lens))


def in_bounds(lay, size_a=None, size_b=None):
    """Every range and the 16 bytes after it lie inside its buffer (of size_a, size_b bytes where the layout does not
    hold the buffers themselves), at a 16-byte aligned offset."""
    lens = lay["lens"].astype(np.int64)
    ok = lambda size, off: bool(np.all(off.astype(np.int64) % 16 == 0) and np.all(off.astype(np.int64) + lens + 16 <= size))
    return ok(len(lay["a"]) if size_a is None else size_a, lay["off_a"]) and ok(len(lay["b"]) if size_b is None else size_b, lay["off_b"])


def report(case, got, limit=8):
    """(length, piece or byte index, got, want) of the first few wrong verdicts."""
    bad = np.flatnonzero(np.asarray(got) != case["expected"])[:limit]
    return [(int(case["lens"][i]), int(case["tag"][i]), int(got[i]), int(case["expected"][i])) for i in bad]


# ---- A, B: one A range, one variant per piece -------------------------------------------------------------------------

A_Q = (1, 2, 255, 256, 257, 767, 768, 769, 1023, 1024, 1025, 1279, 1280, 1281, 1791, 1792, 1793, 2047, 2048, 2049, 2305)
A_LENGTHS = tuple(n for q in A_Q for n in (16 * q, 16 * q + 5))
B_LENGTHS = (CHUNK, CHUNK - 13, CHUNK + 1)


def one_range_case(name, n, pieces, seed):
    """One A range of n bytes (off_a is the same for every pair, off_b walks); one variant per entry of `pieces` with
    one bit flipped at a seeded byte of that piece, and a last variant with nothing flipped.  tag: the piece."""
    rng = np.random.default_rng(seed)
    pieces = np.asarray(pieces, dtype=np.int64)
    valid = np.minimum(PIECE, n - PIECE * pieces)  # the last piece may be partial
    pos = PIECE * pieces + rng.integers(0, valid)
    mask = np.uint8(1) << rng.integers(0, 8, size=len(pieces)).astype(np.uint8)
    k = len(pieces)
    return make_case(name, [n], rng.integers(0, 256, size=n, dtype=np.uint8), np.zeros(k + 1, dtype=np.int64),
                     np.arange(k), pos, mask, np.concatenate((pieces, [-1])), lead=48, n=n, pieces=pieces)


def group_a_case(n):
    return one_range_case("A/%d" % n, n, np.arange((n + 15) // 16), [0xA, n])


def b_pieces(n):
    last = (n + 15) // 16 - 1
    return np.array(sorted(set(range(0, 1031)) | set(range(1031, 15350, 61)) | set(range(15350, last + 1))), dtype=np.int64)


def group_b_case(n):
    return one_range_case("B/%d" % n, n, b_pieces(n), [0xB, n])


# ---- C: the tail mask -------------------------------------------------------------------------------------------------

C_Q = (0, 1, 256, 1024)


def group_c_case():
    """For every q and v = 1..15 an A range of 16 q + v bytes; 32 variants of it: byte j = 0..15 of the last piece,
    bit 0 or 7.  A variant differs iff j < v.  tag: the flipped byte."""
    rng = np.random.default_rng(0xC)
    a_len = [16 * q + v for q in C_Q for v in range(1, 16)]
    src, pos, mask, vs, js = [], [], [], [], []
    for r, (q, v) in enumerate((q, v) for q in C_Q for v in range(1, 16)):
        for j in range(16):
            for bit in (0, 7):
                src.append(r)
                pos.append(16 * q + j)
                mask.append(1 << bit)
                vs.append(v)
                js.append(j)
    return make_case("C", a_len, rng.integers(0, 256, size=sum(a_len), dtype=np.uint8), src, np.arange(len(src)), pos, mask, pos,
                     v=np.array(vs), j=np.array(js))


# ---- D: chunks and the pair a chunk belongs to ------------------------------------------------------------------------

D_SHAPES = (0, CHUNK, 0, 0, 2 * CHUNK + 17, 1, 3 * CHUNK, 0, CHUNK + 1, 16, 3 * CHUNK + 1, 0)


def group_d_cases():
    """-> two cases over the same pairs: in the order of D_SHAPES, and shuffled.  For every shape that is not empty:
    a variant for the byte on each side of every chunk boundary, one for the last byte, one with a flip in every chunk
    at once, one with none; a zero-length pair after every variant and for every empty shape.  tag: the first flipped
    byte."""
    rng = np.random.default_rng(0xD)
    empty = [s for s, n in enumerate(D_SHAPES) if n == 0]
    pairs = []  # (src, [positions])
    for s, n in enumerate(D_SHAPES):
        if n == 0:
            pairs.append((s, []))
            continue
        variants = [[c + d] for c in range(CHUNK, n, CHUNK) for d in (-1, 0)] + [[n - 1]]
        variants.append([c + int(rng.integers(0, min(CHUNK, n - c))) for c in range(0, n, CHUNK)])
        variants.append([])
        for v in variants:
            pairs.append((s, v))
            pairs.append((empty[len(pairs) % len(empty)], []))
    data = rng.integers(0, 256, size=sum(D_SHAPES), dtype=np.uint8)
    out = []
    for name, order in (("D/ordered", range(len(pairs))), ("D/shuffled", np.random.default_rng(0xD5).permutation(len(pairs)))):
        ps = [pairs[i] for i in order]
        fp = [i for i, (_, v) in enumerate(ps) for _ in v]
        fo = [p for _, v in ps for p in v]
        fm = [1 << ((i + p) % 8) for i, p in zip(fp, fo)]
        out.append(make_case(name, D_SHAPES, data, [s for s, _ in ps], fp, fo, fm, [v[0] if v else -1 for _, v in ps], lead=32))
    return out


# ---- E: many small pairs ----------------------------------------------------------------------------------------------

E_PAIRS = 200000


def group_e_case():
    """200 000 pairs of 0..80 bytes, each with an A range of its own; about half carry one flipped bit at a position
    in [0, len + 15): at or past len it lies in the slack and must be ignored.  tag: that position."""
    rng = np.random.default_rng(0xE)
    lens = rng.integers(0, 81, size=E_PAIRS)
    fp = np.flatnonzero(rng.random(E_PAIRS) < 0.5)
    fo = (rng.random(len(fp)) * (lens[fp] + 15)).astype(np.int64)
    fm = np.uint8(1) << rng.integers(0, 8, size=len(fp)).astype(np.uint8)
    tag = np.full(E_PAIRS, -1, dtype=np.int64)
    tag[fp] = fo
    return make_case("E", lens, rng.integers(0, 256, size=int(lens.sum()), dtype=np.uint8), np.arange(E_PAIRS), fp, fo, fm, tag)


# ---- F: aliasing ------------------------------------------------------------------------------------------------------

F_LENGTHS = (1, 15, 16, 17, 0, 4095, 4101, 16 * 768, 16 * 769 + 5, 16 * 1793, CHUNK + 17)


def group_f_cases():
    """-> [(case, layout)]: "F/two_bases": two buffers and off_a != off_b for every pair; "F/one_allocation": the same
    pairs with both sides in one buffer (a is b); "F/self": every range against itself (a is b, off_a == off_b), all
    equal.  The pairs of the first two: each range unflipped, with its first byte, its last byte, and the byte just
    past its end flipped."""
    rng = np.random.default_rng(0xF)
    src, fp, fo, tag = [], [], [], []
    for r, n in enumerate(F_LENGTHS):
        for pos in (None, 0, n - 1, n):
            if pos is not None and pos >= 0:  # (an empty range has no last byte: that variant stays as it is)
                fp.append(len(src))
                fo.append(pos)
            src.append(r)
            tag.append(-1 if pos is None or pos < 0 else pos)
    data = rng.integers(0, 256, size=sum(F_LENGTHS), dtype=np.uint8)
    fm = [0x80 if i % 2 else 0x01 for i in range(len(fp))]
    two = make_case("F/two_bases", F_LENGTHS, data, src, fp, fo, fm, tag, lead=4096 + 16)
    lay = materialise(two)
    assert np.all(lay["off_a"] != lay["off_b"])
    one = dict(two, name="F/one_allocation")
    both = np.concatenate((lay["a"], lay["b"]))
    lay1 = dict(a=both, b=both, off_a=lay["off_a"], off_b=lay["off_b"] + np.uint64(len(lay["a"])), lens=lay["lens"])
    own = make_case("F/self", F_LENGTHS, data, np.arange(len(F_LENGTHS)), [], [], [], [-1] * len(F_LENGTHS), lead=16)
    lay2 = dict(a=own["a"], b=own["a"], off_a=np.ascontiguousarray(own["a_off"], dtype=np.uint64),
                off_b=np.ascontiguousarray(own["a_off"], dtype=np.uint64), lens=np.ascontiguousarray(own["a_len"], dtype=np.uint64))
    return [(two, lay), (one, lay1), (own, lay2)]


# ---- the staged pass of files_equal_impl ------------------------------------------------------------------------------

STAGING = 1 << 16
HALF = STAGING // 2  # H in files_equal_impl for a ctx of this staging: a lone pair is cut at its multiples
LONE_LEN = 5 * HALF + 17
MULTI_LENGTHS = (1, 15, 16, 17, 4095, 32767, 32768, 32769, 70001, 200003)


def lone_pair_flips():
    """The flip of each call on one pair of LONE_LEN bytes: its first and last byte and the three bytes around every
    cut; None: nothing flipped."""
    cuts = range(HALF, LONE_LEN, HALF)
    return [0, LONE_LEN - 1] + [c + d for c in cuts for d in (-1, 0, 1)] + [None]


def multi_pair_plan():
    """-> [(length, flip position or None, mask)] of one call: lengths of MULTI_LENGTHS in seeded order, six of each;
    one third equal, the others with one flipped bit at a seeded position, the last byte for every fifth of them."""
    rng = np.random.default_rng(0x51)
    lens = rng.permutation(np.repeat(MULTI_LENGTHS, 6))
    out, k = [], 0
    for i, n in enumerate(lens.tolist()):
        if i % 3 == 0:
            out.append((n, None, 0))
            continue
        k += 1
        out.append((n, n - 1 if k % 5 == 0 else int(rng.integers(0, n)), 1 << int(rng.integers(0, 8))))
    return out


# ---- fill_synthetic_kernel --------------------------------------------------------------------------------------------

FILL_SPAN = 64 * 256 * 8  # bytes one pass of the grid covers at its cap of 64 blocks: longer files take the stride loop
FILL_BIG_LENGTHS = (FILL_SPAN - 8, FILL_SPAN, FILL_SPAN + 8) + tuple(range(FILL_SPAN + 1, FILL_SPAN + 8)) + (3 * FILL_SPAN + 5,) + \
    tuple((1 << 20) + k for k in range(8))
FILL_BIG_INDEX = tuple((1 << 32) + i for i in range(len(FILL_BIG_LENGTHS) - 2)) + ((1 << 63) + 5, (1 << 64) - 1)
FILL_SLICE = 65535  # files per launch (gridDim.y)
FILL_MANY = (FILL_SLICE, FILL_SLICE + 1, FILL_SLICE + 2 + 3)


def fill_many(n):
    """-> lens, file_index of a list of n files whose lengths cycle through 0..17 and whose indices cross 2**32."""
    i = np.arange(n, dtype=np.uint64)
    return i % np.uint64(18), np.uint64((1 << 32) - 40000) + i
