"""Block mode of the install side on the CPU (SNAPHASH_FLAG_SPLIT_BLOCKS): the block scan's checker
(inflate_core.h inf_dynamic_ok) against inf_dynamic at every bit offset, inflate_run's block stop rule against a serial
walk that records every block, and the whole block mode run serially (tests/inflate_blocks_harness.cpp: scan, decode of
every candidate into a hole slot, link, fill, the host taking a block where the chain breaks) against Python's zlib.
The GPU kernels that run the same code are checked in tests/test_gpu_inflate_blocks.py."""
import ctypes
import functools
import gzip
import os
import random
import zlib

import numpy as np
import pytest

import hostbuild
from conftest import ROOT

EFORMAT = -9
K_BLOCK, K_FINAL, K_OVERFLOW, K_TRUNCATED = 5, 0, 3, 2
NO_STOP = (1 << 64) - 1
STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "filtered": zlib.Z_FILTERED, "huffman": zlib.Z_HUFFMAN_ONLY, "rle": zlib.Z_RLE,
              "fixed": zlib.Z_FIXED}
u64 = ctypes.c_uint64
P = ctypes.POINTER


class BlockStats(ctypes.Structure):
    _fields_ = [(f, u64) for f in ("pieces", "candidates", "linked", "linked_from_block", "host_blocks", "host_bytes")]


@functools.lru_cache(maxsize=None)
def load_blocks():
    """tests/inflate_blocks_harness.cpp, loaded once a process with every prototype (it keeps no state between calls)."""
    L = hostbuild.shared("tests/inflate_blocks_harness.cpp")
    cp, sz = ctypes.c_char_p, ctypes.c_size_t
    L.ibh_dynamic_ref.argtypes = [cp, sz, u64]
    L.ibh_dynamic_ok.argtypes = [cp, sz, u64]
    L.ibh_diff.argtypes = [cp, sz, P(u64), P(u64)]
    L.ibh_diff.restype = u64
    L.ibh_scan.argtypes = [cp, sz, P(u64), sz]
    L.ibh_scan.restype = sz
    L.ibh_blocks.argtypes = [cp, sz, P(u64), P(ctypes.c_uint32), P(u64), sz, P(u64)]
    L.ibh_blocks.restype = ctypes.c_long
    L.ibh_segment.argtypes = [cp, sz, u64, sz, u64, P(ctypes.c_int), P(u64), P(u64), P(ctypes.c_uint32)]
    L.ibh_gunzip_blocks.argtypes = [cp, sz, sz, ctypes.c_uint32, u64, P(ctypes.c_void_p), P(sz), P(BlockStats)]
    L.ibh_free.argtypes = [ctypes.c_void_p]
    return L


@pytest.fixture(scope="module")
def bh():
    return load_blocks()


def raw_deflate(data, level=9, strategy=zlib.Z_DEFAULT_STRATEGY, mem=8):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    return c.compress(data) + c.flush()


def diff(L, buf):
    acc, first = u64(), u64()
    bad = L.ibh_diff(buf, len(buf), ctypes.byref(acc), ctypes.byref(first))
    return bad, acc.value, first.value


def blocks(L, raw):
    cap = 1 << 16
    st, ty, ol, end = (u64 * cap)(), (ctypes.c_uint32 * cap)(), (u64 * cap)(), u64()
    k = L.ibh_blocks(raw, len(raw), st, ty, ol, cap, ctypes.byref(end))
    assert 0 <= k <= cap
    return [(st[i], ty[i], ol[i]) for i in range(k)], end.value


def scan(L, buf):
    cap = 1 << 16
    out = (u64 * cap)()
    k = L.ibh_scan(buf, len(buf), out, cap)
    return list(out[:min(k, cap)])


def segment(L, raw, start, cap, block_min):
    cut, end, n, he = ctypes.c_int(), u64(), u64(), ctypes.c_uint32()
    st = L.ibh_segment(raw, len(raw), start, cap, block_min, ctypes.byref(cut), ctypes.byref(end), ctypes.byref(n), ctypes.byref(he))
    return st, cut.value, end.value, n.value, he.value


def gunzip_blocks(L, gz, piece=1 << 20, slot=320 << 10, block_min=16384):
    p, n, st = ctypes.c_void_p(), ctypes.c_size_t(), BlockStats()
    rc = L.ibh_gunzip_blocks(gz, len(gz), piece, slot, block_min, ctypes.byref(p), ctypes.byref(n), ctypes.byref(st))
    out = ctypes.string_at(p.value, n.value) if p.value else b""
    if p.value:
        L.ibh_free(p)
    return rc, out, {f: getattr(st, f) for f, _ in BlockStats._fields_}


def corpus(kind, n, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
    if kind == "sources":
        src = open(os.path.join(ROOT, "snappy_amd", "csrc", "snaphash_api.cpp"), "rb").read()
        return (src * (n // len(src) + 1))[:n]
    words = [bytes(rng.integers(97, 123, size=int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(1500)]
    return b" ".join(words[int(i)] for i in rng.zipf(1.3, size=n // 4 + 8) % 1500)[:n]


def mixed(n, seed):
    return corpus("text", n // 2, seed) + corpus("random", n // 6, seed + 1) + corpus("sources", n - n // 2 - n // 6, seed)


# ---- the checker ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("level", [1, 6, 9])
@pytest.mark.parametrize("strategy", sorted(STRATEGIES))
def test_checker_equals_inf_dynamic_at_every_bit(bh, level, strategy):
    raw = raw_deflate(mixed(150000, level), level, STRATEGIES[strategy])
    bad, acc, first = diff(bh, raw)
    assert bad == 0, "checker and inf_dynamic differ first at bit %d" % first
    # every true dynamic block start (the serial walk's) is accepted
    bl, _ = blocks(bh, raw)
    dyn = [s for s, t, _ in bl if t == 2]
    got = set(scan(bh, raw))
    assert all(s in got for s in dyn), (len(dyn), len(got))
    if strategy == "fixed":
        assert not dyn
    else:
        assert dyn and acc >= len(dyn)


def test_checker_on_random_bytes(bh):
    for seed in range(6):
        buf = corpus("random", 60000, seed)
        bad, acc, first = diff(bh, buf)
        assert bad == 0, (seed, first)


def test_checker_on_near_misses(bh):
    """Single bits flipped in true headers -- HLIT, HDIST, HCLEN, the precode, the repeat codes, the code lengths and the
    EOB length: the checker must still say what inf_dynamic says, at the header's start and around it."""
    rng = random.Random(3)
    raw = bytearray(raw_deflate(corpus("text", 600000, 2) + corpus("random", 20000, 4), 9))
    bl, _ = blocks(bh, bytes(raw))
    starts = [s for s, t, _ in bl if t == 2][:6]
    assert len(starts) >= 3
    accepted = rejected = 0
    for s in starts:
        for k in list(range(1, 120)) + rng.sample(range(120, 2000), 150):  # the header bits, and a sample of the lengths
            m = bytearray(raw)
            m[(s + k) >> 3] ^= 1 << ((s + k) & 7)
            lo, hi = max(0, (s >> 3) - 4), min(len(m), (s >> 3) + 400)
            win = bytes(m[lo:hi])
            for b in range(max(0, s - lo * 8 - 9), s - lo * 8 + 9):
                a, r = bh.ibh_dynamic_ok(win, len(win), b), bh.ibh_dynamic_ref(win, len(win), b)
                assert a == r, (s, k, b)
            at = s - lo * 8
            if bh.ibh_dynamic_ref(win, len(win), at):
                accepted += 1
            else:
                rejected += 1
    assert accepted > 50 and rejected > 300, (accepted, rejected)  # both answers were exercised


def test_checker_needs_the_whole_header_in_the_piece(bh):
    raw = raw_deflate(corpus("text", 400000, 7), 9)
    s = [b for b, t, _ in blocks(bh, raw)[0] if t == 2][1]
    whole = bh.ibh_dynamic_ok(raw, len(raw), s)
    assert whole
    for cut in range((s >> 3) + 1, (s >> 3) + 400, 7):
        assert bh.ibh_dynamic_ok(raw[:cut], cut, s) == bh.ibh_dynamic_ref(raw[:cut], cut, s)
    assert not bh.ibh_dynamic_ok(raw[:(s >> 3) + 20], (s >> 3) + 20, s)


# ---- the stop rule ------------------------------------------------------------------------------------------------------

def test_block_stop_ends_at_the_recorded_block_ends(bh):
    raw = raw_deflate(corpus("text", 400000, 1) + corpus("random", 40000, 2) + corpus("sources", 200000, 3), 6)
    bl, end = blocks(bh, raw)
    assert len(bl) >= 8
    ends = [bl[i + 1][0] for i in range(len(bl) - 1)] + [end]
    starts = {s: i for i, (s, _, _) in enumerate(bl)}
    # from every block start with block_min = 0: one block, or on through the blocks a segment cannot start at
    for i, (s, t, o) in enumerate(bl):
        st, cut, e, n, he = segment(bh, raw, s, 1 << 20, 0)
        assert cut == 0 and he <= n
        if st == K_FINAL:
            assert e == end
            continue
        assert st == K_BLOCK and e in starts and e in ends, (i, st, e)
        j = starts[e]
        assert j > i and n == sum(x[2] for x in bl[i:j])
        # it stopped where a dynamic block follows or a stored one ended, and nowhere before
        assert bl[j][1] == 2 or bl[j - 1][1] == 0
        assert all(bl[q][1] != 2 and bl[q - 1][1] != 0 for q in range(i + 1, j))
    # block_min: the first such end at or after it
    st, cut, e, n, he = segment(bh, raw, 0, 1 << 22, 200000)
    assert st == K_BLOCK and n >= 200000 and e in starts
    j = starts[e]
    assert sum(x[2] for x in bl[:j - 1]) < 200000 or bl[j - 1][1] != 2


def test_flush_mode_is_unchanged_by_block_mode(bh):
    raw = raw_deflate(corpus("text", 200000, 5), 9)
    st, cut, e, n, he = segment(bh, raw, 0, 1 << 22, NO_STOP)
    assert st == K_FINAL and n == 200000 and cut == 0


def test_overflow_rolls_back_to_the_last_block_end(bh):
    raw = raw_deflate(corpus("text", 600000, 9), 9)
    bl, _ = blocks(bh, raw)
    o1, o2 = bl[0][2], bl[1][2]
    st, cut, e, n, he = segment(bh, raw, 0, o1 + o2 // 2, 1 << 30)
    assert (st, cut, e, n) == (K_BLOCK, K_OVERFLOW, bl[1][0], o1) and he <= n
    # a later start: its holes end inside the block it kept
    st, cut, e, n, he = segment(bh, raw, bl[2][0], bl[2][2] + bl[3][2] // 3, 1 << 30)
    assert (st, cut, e, n) == (K_BLOCK, K_OVERFLOW, bl[3][0], bl[2][2]) and 0 < he <= n
    # a single block that does not fit is a plain overflow
    st, cut, e, n, he = segment(bh, raw, bl[2][0], bl[2][2] - 1, 0)
    assert st == K_OVERFLOW and cut == 0
    # the input ends inside the second block: cut back to the first
    piece = raw[: (bl[1][0] >> 3) + 3000]
    st, cut, e, n, he = segment(bh, piece, 0, 1 << 22, 1 << 30)
    assert (st, cut, e, n) == (K_BLOCK, K_TRUNCATED, bl[1][0], o1)


# ---- the whole block mode, serially ------------------------------------------------------------------------------------

def check(bh, gz, want, **kw):
    rc, out, st = gunzip_blocks(bh, gz, **kw)
    assert rc == 0 and out == want, (rc, len(out), len(want), st)
    return st


def test_plain_zlib_streams_link_from_block_candidates(bh):
    data = corpus("text", 3 << 20, 11)
    for level in (1, 6, 9):
        st = check(bh, gzip.compress(data, level), data)
        assert st["host_blocks"] == 0 and st["linked_from_block"] >= 20, st
        assert st["linked"] == st["linked_from_block"], st  # (the member's first block is a dynamic one too)


def test_random_streams(bh):
    rng = random.Random(17)
    for i in range(220):
        kind = rng.choice(["text", "sources", "random", "mixed", "short"])
        n = rng.choice([0, 1, 2, 100, 5000, 40000, 150000, 400000])
        data = mixed(n, i) if kind == "mixed" else (corpus("text", n, i)[: rng.randint(0, 300)] if kind == "short" else corpus(kind, n, i))
        level = rng.choice([1, 6, 9])
        strategy = rng.choice(list(STRATEGIES.values()))
        c = zlib.compressobj(level, zlib.DEFLATED, 31, rng.choice([1, 8, 9]), strategy)
        gz = c.compress(data) + c.flush()
        piece = rng.choice([1 << 20, 60000, 20000])
        check(bh, gz, data, piece=piece, block_min=rng.choice([0, 16384, 100000]))


def test_all_fixed_stream_goes_to_the_host_a_block_at_a_time(bh):
    # no candidates: the piece's first segment runs on through fixed blocks until its slot is full, then the host takes
    # the stretch (the rest of the member: no block the scan can find follows); the bytes are the same
    data = corpus("text", 1200000, 21)
    c = zlib.compressobj(9, zlib.DEFLATED, 31, 8, zlib.Z_FIXED)
    gz = c.compress(data) + c.flush()
    st = check(bh, gz, data)
    assert st["candidates"] == 0 and st["host_blocks"] >= 1 and st["host_bytes"] > 0
    st = check(bh, gz, data, slot=1 << 22)  # a slot that holds it all: one segment
    assert st["candidates"] == 0 and st["host_blocks"] == 0 and st["linked"] == 1


def test_incompressible_data_is_stored_blocks(bh):
    data = corpus("random", 500000, 22)
    st = check(bh, gzip.compress(data, 9), data, piece=100000)
    assert st["host_blocks"] == 0 and st["linked"] >= 5, st


def test_first_block_fixed_then_dynamic(bh):
    # a short first block (zlib picks fixed codes for it), a full flush, then long dynamic blocks
    data = corpus("text", 400000, 23)
    c = zlib.compressobj(9, zlib.DEFLATED, 31)
    gz = c.compress(data[:40]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[40:]) + c.flush()
    raw = gz[10:-8]
    bl, _ = blocks(bh, raw)
    assert bl[0][1] == 1 and any(t == 2 for _, t, _ in bl)
    check(bh, gz, data)
    check(bh, gz, data, block_min=0, piece=30000)


def test_final_dynamic_block_at_odd_bit(bh):
    found = False
    for seed in range(40):
        data = corpus("text", 70000 + 997 * seed, seed)
        gz = gzip.compress(data, 9)
        bl, _ = blocks(bh, gz[10:-8])
        if bl[-1][1] == 2 and bl[-1][0] % 8 in (1, 3, 5, 7):
            found = True
            check(bh, gz, data, block_min=0)
    assert found


def test_empty_one_byte_and_concatenated_members(bh):
    check(bh, gzip.compress(b"", 9), b"")
    check(bh, gzip.compress(b"x", 9), b"x")
    a, b = corpus("text", 300000, 31), corpus("sources", 200000, 32)
    # the library's producer writes flush points; plain zlib does not: one member of each, and empty ones between
    sync = zlib.compressobj(6, zlib.DEFLATED, 31)
    prod = b"".join(sync.compress(a[i:i + 65536]) + sync.flush(zlib.Z_SYNC_FLUSH) for i in range(0, len(a), 65536)) + sync.flush()
    gz = prod + gzip.compress(b"", 9) + gzip.compress(b, 9) + gzip.compress(b"y", 1)
    check(bh, gz, a + b + b"y", piece=70000)


def test_block_larger_than_a_slot_goes_to_the_host(bh):
    data = corpus("text", 600000, 41)
    gz = gzip.compress(data, 9)
    st = check(bh, gz, data, slot=30000)
    assert st["host_blocks"] >= 1
    zeros = bytes(3 << 20)  # zlib -9 on zeros: blocks of megabytes
    st = check(bh, gzip.compress(zeros, 9), zeros)
    assert st["host_blocks"] >= 1


def test_corrupt_streams_are_eformat(bh):
    data = corpus("text", 300000, 51)
    gz = bytearray(gzip.compress(data, 9))
    rng = random.Random(5)
    for _ in range(25):
        m = bytearray(gz)
        k = rng.randrange(12, len(m) - 8)
        m[k] ^= 1 << rng.randrange(8)
        rc, out, _ = gunzip_blocks(bh, bytes(m))
        assert rc == EFORMAT or out == data  # (a flip in an unused bit decodes the same; the CRC catches the rest)
    rc, _, _ = gunzip_blocks(bh, bytes(gz[:-30]))
    assert rc == EFORMAT
    rc, _, _ = gunzip_blocks(bh, bytes(gz[:len(gz) // 2]))
    assert rc == EFORMAT
    rc, _, _ = gunzip_blocks(bh, b"")
    assert rc == EFORMAT
