"""The edge streams of tests/inflate_edge_streams.py on the CPU: zlib decodes each one (or refuses it where it is meant to
be invalid), the host harnesses of inflate_core.h agree, and -- read from the harnesses' view, not assumed -- every
stream has the shape it claims, so that a failure of tests/test_gpu_inflate_edges.py points at the kernels or at
unpack.inc.  The items, and the code each one reaches:
  1  hole fill at the format's limits           inflate_fill_kernel, gpu_fill_concat
  2  hole fill, segment lookup                  inflate_fill_kernel's walk back over short and empty segments
  3  the window in front of a piece             d_win, wlen; a member's start with another member's bytes in front of it
  4  false and too many flush candidates        inflate_scan_kernel, cand_cap, the cut to the launch's slots
  5  slot capacity                              kInflateSlotSyms, kInfOverflow, the host's stretches; block slots
  6  pieces that end inside a segment           kInfTruncated, pos >= pn
  7  the decode routine as the device runs it   inflate_decode_kernel on block types and codes the corpora never have
  8  the block scan at tile, halo, piece edges  inflate_block_scan_kernel"""
import ctypes
import zlib

import numpy as np
import pytest

import inflate_edge_streams as E
from test_inflate_blocks_host import bh, blocks, gunzip_blocks, scan  # noqa: F401  (bh: a fixture)
from test_inflate_host import EFORMAT, _take, gunzip, ih, inflate_raw, segments  # noqa: F401  (ih: a fixture)

K_FINAL, K_FLUSH, K_OVERFLOW = 0, 1, 3


def gunzip_all(gz):
    """Every member of gz through zlib (the reference of this file and of the GPU file)."""
    out = b""
    while gz:
        d = zlib.decompressobj(31)
        out += d.decompress(gz)
        assert d.eof
        gz = d.unused_data
    return out


def segment(L, raw, start, cap=1 << 20):
    """One segment from byte `start` in hole mode, as the kernel decodes it: status, symbols, end byte, hole_end."""
    n, st, end, he = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_uint64(), ctypes.c_uint32()
    p = L.ih_segment(raw, len(raw), start * 8, cap, ctypes.byref(n), ctypes.byref(st), ctypes.byref(end), ctypes.byref(he))
    syms = np.frombuffer(_take(L, p, 2 * n.value), dtype=np.uint16)
    return st.value, syms, end.value // 8, he.value


def walk(L, r, cap=1 << 20):
    """The stream's segments as the harness sees them from the builder's starts: every one must end where the next
    starts.  -> [(status, symbols, hole_end)]"""
    out = []
    for i, s in enumerate(r["starts"]):
        st, syms, end, he = segment(L, r["raw"], s, cap)
        last = i + 1 == len(r["starts"])
        assert st == (K_FINAL if last else K_FLUSH), (i, st)
        assert last or end == r["starts"][i + 1], i
        assert len(syms) == r["lens"][i], (i, len(syms), r["lens"][i])
        out.append((st, syms, he))
    return out


def candidates(L, raw):
    k = L.ih_candidates(raw, len(raw), None, 0)
    c = (ctypes.c_uint64 * max(k, 1))()
    L.ih_candidates(raw, len(raw), c, k)
    return list(c[:k])


def agrees(L, r):
    """zlib, the serial host decoder and the segmented one give the builder's bytes."""
    assert gunzip_all(r["gz"]) == r["data"]
    assert gunzip(L, r["gz"]) == (0, r["data"])
    if "starts" in r:
        assert segments(L, r["raw"], r["starts"]) == (0, r["data"])
        assert set(r["starts"][1:]) <= set(candidates(L, r["raw"]))
        assert E.flush_candidates(r["raw"]) == candidates(L, r["raw"])  # (the restatement plan_flush relies on)


def kernel_only(r):
    """What the GPU file asserts host_bytes == 0 for: every segment fits a slot."""
    return max(r["lens"]) <= E.SLOT_SYMS


def test_item1_every_symbol_a_far_hole_of_a_hole(ih):
    r = E.far_hole_chain()
    agrees(ih, r)
    segs = walk(ih, r)
    assert len(segs) >= 3 * (E.WINDOW // r["seg_len"] + 1)  # holes of holes of holes
    for st, syms, he in segs[1:-1]:
        assert len(syms) == r["seg_len"] < E.WINDOW and np.all(syms >= 256) and he == len(syms)
        assert syms.max() == syms[0] == 256 + E.WINDOW == 256 + r["far"]
    assert kernel_only(r)


def test_item2_holes_across_tiny_and_empty_segments(ih):
    r = E.tiny_segments()
    agrees(ih, r)
    segs = walk(ih, r)
    lens = [len(s[1]) for s in segs]
    assert {0, 1, 2, 3} <= set(lens) and any(lens[i] == lens[i + 1] == 0 for i in range(len(lens) - 1))
    for i, dist in r["far"]:
        syms = segs[i][1]
        assert syms[0] == 256 + dist and dist > sum(lens[i - 6:i]) >= 6 and lens[i - 1] == lens[i - 2] == 0
        # consecutive holes of the one match: their bytes lie in four or more different segments
        src = {next(k for k in range(i - 1, -1, -1) if sum(lens[k:i]) >= int(v) - 256) for v in syms[:46]}
        assert len(src) >= 4, src
        assert np.all(segs[i + 1][1][:20] >= 256)  # and the next segment copies holes
    assert kernel_only(r)


@pytest.mark.parametrize("first", [50000, 20000])
def test_item3_window_in_front_of_a_piece(ih, first):
    r = E.window_edge(first)
    agrees(ih, r)
    segs = walk(ih, r)
    assert r["wlen"] == min(first, E.WINDOW) and segs[1][1][0] == 256 + r["wlen"]
    assert 256 + 1 in segs[1][1][:300]  # the window's newest byte
    if first < E.WINDOW:  # one byte further is in front of the member: zlib and the host decoder refuse it
        bad = E.window_edge(first, 1)
        assert bad["data"] is None
        with pytest.raises(zlib.error, match="too far back"):
            zlib.decompress(bad["gz"], 31)
        assert gunzip(ih, bad["gz"])[0] == EFORMAT
        assert segments(ih, bad["raw"], bad["starts"])[0] == EFORMAT
        assert segment(ih, bad["raw"], bad["starts"][1])[1][0] == 256 + first + 1


@pytest.mark.parametrize("lead, pad", [(0, 0), (10, 0), (0, 1100 << 10)])
def test_item3_reference_in_front_of_a_later_member(ih, bh, lead, pad):
    r = E.reach_before_member(lead, pad)
    with pytest.raises(zlib.error, match="too far back"):
        gunzip_all(r["gz"])
    assert gunzip_all(r["good"]["gz"]) == r["good"]["data"] and len(r["good"]["data"]) >= lead + 100
    assert gunzip(ih, r["gz"])[0] == EFORMAT
    assert gunzip_blocks(bh, r["gz"])[0] == EFORMAT
    assert (len(r["raw"]) >= E.SPLIT_MIN) == bool(pad)


def test_item4_more_false_candidates_than_the_scan_keeps(ih):
    r = E.dense_false_candidates()
    agrees(ih, r)
    walk(ih, r)
    cand = candidates(ih, r["raw"])
    assert len(cand) > len(r["raw"]) // 4 + 16 and len(cand) > 4096  # cand_cap, and any launch's slots
    first_piece = [c for c in cand if c <= E.PIECE_FLOOR]
    assert len(first_piece) > E.PIECE_FLOOR // 4 + 16


@pytest.mark.parametrize("kind", sorted(E.SLOT_PATTERNS))
def test_item5_segments_at_the_slot_capacity(ih, kind):
    r = E.slot_capacity(kind)
    agrees(ih, r)
    walk(ih, r)
    assert r["lens"][:-1] == E.SLOT_PATTERNS[kind]
    for s, n in zip(r["starts"], r["lens"]):  # as the kernel decodes it, into a slot
        st = segment(ih, r["raw"], s, E.SLOT_SYMS)[0]
        assert (st == K_OVERFLOW) == (n > E.SLOT_SYMS), (n, st)
    want = {"exact": (6, 0), "one_over": (1, 5 * (E.SLOT_SYMS + 1)),
            "alternating": (9, 3 * (E.SLOT_SYMS + 1) + E.SLOT_SYMS + 2 + 70000)}[kind]
    assert E.plan_flush(r["gz"][10:], r["starts"], r["lens"], 8 << 20) == want


@pytest.mark.parametrize("rle", [False, True])
def test_item5_block_longer_than_a_block_slot(bh, rle):
    r = E.long_block(rle)
    assert gunzip_all(r["gz"]) == r["data"]
    bl, _ = blocks(bh, r["raw"])
    assert max(o for _, _, o in bl) > 3 * E.BLOCK_SLOT_SYMS and len(r["raw"]) >= E.SPLIT_MIN
    rc, out, st = gunzip_blocks(bh, r["gz"])
    assert rc == 0 and out == r["data"]
    assert st["host_blocks"] >= 1 and st["host_bytes"] >= sum(o for _, _, o in bl if o > E.BLOCK_SLOT_SYMS)


@pytest.mark.parametrize("kind, want", [("level0", (1, 6 * 65535)), ("on_piece_end", (6, 0)), ("final_on_piece_end", (4, 0))])
def test_item6_pieces_that_end_inside_or_on_a_segment(ih, kind, want):
    r = E.piece_cuts(kind)
    agrees(ih, r)
    walk(ih, r)
    z = r["gz"][10:]
    ends = r["starts"][1:] + [len(r["raw"])]
    if kind == "level0":
        assert all(e - s == E.PIECE_FLOOR + 4 for s, e in zip(r["starts"][:-1], ends))
    else:
        assert all(e % E.PIECE_FLOOR == 0 for e in ends[:4])
        assert (len(r["raw"]) % E.PIECE_FLOOR == 0) == (kind == "final_on_piece_end")
    assert E.plan_flush(z, r["starts"], r["lens"], E.PIECE_FLOOR) == want
    assert E.plan_flush(z, r["starts"], r["lens"], 8 << 20) == (len(r["lens"]), 0)  # (host threads: pieces of 8 MiB)


def test_item7_block_types_and_codes_the_corpora_never_have(ih, bh):
    streams = E.decode_streams()
    for name, r in streams.items():
        agrees(ih, r)
        walk(ih, r, E.SLOT_SYMS)  # every segment fits a slot: the kernel's
        assert kernel_only(r) and len(r["lens"]) >= 4, name
    types = {name: {t for _, t, _ in blocks(bh, r["raw"])[0]} for name, r in streams.items()}
    assert types["fixed"] == {0, 1} and types["huffman_only"] == {0, 2} and 2 in types["long_codes"]
    assert streams["long_codes"]["lit_max"] == streams["long_codes"]["dist_max"] == 15
    for name, d in (("distance_1", [1]), ("distance_15_16", [15, 16]), ("distance_17", [17, 18])):
        assert streams[name]["dists"] == d and streams[name]["dist_codes"] == 1 and types[name] == {0, 2}
    # zlib at wbits 9 never reaches further back than its window of 512
    r = streams["wbits9"]
    d = zlib.decompressobj(-9)
    assert d.decompress(r["raw"]) == r["data"]
    # Z_HUFFMAN_ONLY: no match at all, so no hole either
    assert all(he == 0 for _, _, he in walk(ih, streams["huffman_only"]))


def scan_pieces(L, r):
    """scan() on each piece the library's scan sees."""
    return [scan(L, r["gz"][a:a + n]) for a, n in r["pieces"]]


def planted(r, piece=0, kinds=("min", "long")):
    a = r["pieces"][piece][0] - 10
    return [b - 8 * a for b, k in r["plants"] if k in kinds and b >= 8 * a]


def test_item8_planted_headers_are_what_the_checker_finds(bh):
    assert E.header_bits("long")[1] == 2233 <= E.HEADER_MAX_BITS and E.header_bits("min")[1] == 91
    assert 8 * (E.SCAN_TILE - 1) + 7 + 2233 + 64 <= 8 * (E.SCAN_TILE + E.SCAN_HALO)  # the long header needs the halo
    edge = 8 * E.SCAN_TILE * E.SCAN_EDGE_TILE
    for make, deltas in ((E.scan_edge, (-16, -1, 0, 15)), (E.scan_halo, (-2, -1, 0, 1))):
        for d in deltas:
            r = make(d)
            assert gunzip_all(r["gz"]) == r["data"]
            assert scan_pieces(bh, r) == [[edge + d]] == [planted(r)], d
    for d, found in ((-9, 1), (-1, 1), (0, 1), (1, 0)):
        r = E.scan_piece_end(d)
        assert gunzip_all(r["gz"]) == r["data"]
        got = scan_pieces(bh, r)[0]
        assert got == planted(r)[:found] and (not found or got[0] + 2233 == 8 * E.SPLIT_MIN + d), d


def test_item8_dense_stretches(bh):
    r = E.scan_dense()
    assert gunzip_all(r["gz"]) == r["data"]
    got = scan_pieces(bh, r)[0]
    assert set(planted(r)) <= set(got) and len(got) >= 600
    piece = r["gz"][10:10 + E.SPLIT_MIN]
    q0 = planted(r)[0]  # the stretch starts on a tile's first bit: its first quarter
    assert q0 % (8 * E.SCAN_TILE) == 0
    heads = sum(E.head_ok(piece, b) for b in range(q0, q0 + 2 * E.SCAN_TILE))
    assert heads > 2 * 64 and heads > 2 * sum(q0 <= b < q0 + 2 * E.SCAN_TILE for b in got)  # most of the queue is refused
    r = E.scan_overflow()
    assert gunzip_all(r["gz"]) == r["data"]
    got = scan_pieces(bh, r)[0]
    assert set(planted(r)) <= set(got) and len(got) > E.SPLIT_MIN // 64 + 4096  # bcand_cap


@pytest.mark.parametrize("length", E.SCAN_TAILS)
def test_item8_second_piece_of_any_length(bh, length):
    r = E.scan_tail(length)
    assert gunzip_all(r["gz"]) == r["data"]
    assert r["pieces"][1][1] == length and r["pieces"][1][0] + length == len(r["gz"])
    first, second = scan_pieces(bh, r)
    assert first == [] and sorted(planted(r, 1)) == second and len(second) == 4
    rc, out, st = gunzip_blocks(bh, r["gz"])
    assert rc == 0 and out == r["data"] and st["pieces"] == 2 and st["candidates"] == 4
