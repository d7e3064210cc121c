"""data.tar.bz2 on the CPU: the bzip2 decoder (snappy_amd/csrc/bzip2_core.h, bzip2_host.cpp) checked against Python's
bz2 (libbz2) -- every level, RLE1 at its edges, concatenated streams, blocks that are periodic after RLE1 -- its
block-parallel form on host threads against the serial decode, the block scan, the rules that make a stream
SNAPHASH_EFORMAT (those of Go's compress/bzip2), and the kernels' sampled inverse BWT (bzip2_core.h's bz_samples ..
bz_sample_write, run serially) against the serial walk.  The GPU kernels that run the same routines are checked in
tests/test_gpu_bunzip2.py and tests/test_gpu_bzip2_edges.py."""
import bz2
import ctypes
import functools
import random

import numpy as np
import pytest

import hostbuild

EFORMAT = -9
BLOCK_MAGIC = 0x314159265359


@functools.lru_cache(maxsize=None)
def load_bzip2():
    """tests/bzip2_host_harness.cpp, loaded once a process with every prototype (it keeps no state between calls)."""
    L = hostbuild.shared("tests/bzip2_host_harness.cpp")
    P = ctypes.POINTER
    L.bh_serial.argtypes = [ctypes.c_char_p, ctypes.c_size_t, P(ctypes.c_size_t), P(ctypes.c_int), P(ctypes.c_uint64)]
    L.bh_serial.restype = ctypes.c_void_p
    L.bh_threads.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint, P(ctypes.c_size_t), P(ctypes.c_int), P(ctypes.c_uint64)]
    L.bh_threads.restype = ctypes.c_void_p
    L.bh_link.argtypes = [ctypes.c_char_p, ctypes.c_size_t, P(ctypes.c_uint64), ctypes.c_size_t, ctypes.c_uint, P(ctypes.c_size_t),
                          P(ctypes.c_int)]
    L.bh_link.restype = ctypes.c_void_p
    L.bh_candidates.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, P(ctypes.c_uint64)]
    L.bh_candidates.restype = ctypes.c_uint64
    L.bh_chain.argtypes = [ctypes.c_char_p, ctypes.c_size_t, P(ctypes.c_uint64), ctypes.c_size_t]
    L.bh_chain.restype = ctypes.c_int64
    L.bh_crc.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    L.bh_crc.restype = ctypes.c_uint32
    L.bh_free.argtypes = [ctypes.c_void_p]
    L.bh_block_bwt.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_char_p, P(ctypes.c_uint32)]
    L.bh_block_bwt.restype = ctypes.c_int64
    L.bh_ibwt.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p]
    L.bh_ibwt.restype = None
    L.bh_ibwt_sampled.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p, P(ctypes.c_uint32)]
    L.bh_ibwt_sampled.restype = ctypes.c_int
    return L


@pytest.fixture(scope="module")
def bh():
    return load_bzip2()


def _take(L, p, n):
    b = ctypes.string_at(p, n)
    L.bh_free(p)
    return b


def serial(L, z):
    n, rc, b = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_uint64()
    out = _take(L, L.bh_serial(z, len(z), ctypes.byref(n), ctypes.byref(rc), ctypes.byref(b)), n.value)
    return rc.value, out


def threads(L, z, t=4):
    n, rc, b = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_uint64()
    out = _take(L, L.bh_threads(z, len(z), t, ctypes.byref(n), ctypes.byref(rc), ctypes.byref(b)), n.value)
    return rc.value, out


def link(L, z, cand, t=3):
    arr = (ctypes.c_uint64 * max(len(cand), 1))(*cand)
    n, rc = ctypes.c_size_t(), ctypes.c_int()
    out = _take(L, L.bh_link(z, len(z), arr, len(cand), t, ctypes.byref(n), ctypes.byref(rc)), n.value)
    return rc.value, out


def candidates(L, z, cap=1 << 16):
    arr = (ctypes.c_uint64 * cap)()
    total = L.bh_candidates(z, len(z), cap, arr)
    return total, list(arr[: min(total, cap)])


def chain(L, z):
    arr = (ctypes.c_uint64 * 4096)()
    k = L.bh_chain(z, len(z), arr, 4096)
    assert k >= 0, k
    return list(arr[:k])


def both(L, z):
    """The serial decode and the threaded one must agree; returns (rc, out)."""
    a, b = serial(L, z), threads(L, z)
    assert a[0] == b[0] and (a[0] != 0 or a[1] == b[1])
    return a


def text(n, seed=0):
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, size=int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(1500)]
    base = b" ".join(words[int(i)] for i in rng.integers(0, 1500, size=n // 5 + 10))
    return base[:n]


def test_empty_and_one_byte(bh):
    for d in (b"", b"x", b"\0"):
        for lv in (1, 9):
            assert both(bh, bz2.compress(d, lv)) == (0, d)


def test_every_level_and_every_byte_value(bh):
    d = text(400000, 1) + bytes(range(256)) * 40 + bytes(range(255, -1, -1)) * 7
    for lv in range(1, 10):
        assert both(bh, bz2.compress(d, lv)) == (0, d), lv


def test_rle1_edges(bh):
    r = random.Random(3)
    for k in (1, 2, 3, 4, 5, 6, 7, 8, 9, 255, 256, 257, 258, 259, 260, 1000, 4096):
        for v in (0, 0x41, 0xff):
            d = bytes([v]) * k
            assert both(bh, bz2.compress(d, 9)) == (0, d), (k, v)
            d2 = b"ab" + bytes([v]) * k + b"c" + bytes([v ^ 1]) * (k + 1)
            assert both(bh, bz2.compress(d2, 1)) == (0, d2), (k, v)
    parts = []
    for _ in range(3000):
        parts.append(bytes([r.randrange(4)]) * r.choice([1, 2, 3, 4, 5, 8, 250, 259, 300]))
    d = b"".join(parts)
    for lv in (1, 9):
        assert both(bh, bz2.compress(d, lv)) == (0, d)


def test_random_text_and_zeros(bh):
    rnd = np.random.default_rng(5).integers(0, 256, size=1 << 20, dtype=np.uint8).tobytes()
    t = text(3 << 20, 6)
    for d in (rnd, t):
        for lv in (1, 9):
            assert both(bh, bz2.compress(d, lv)) == (0, d)
    # one block of near-maximal expansion: 43 MiB of zeros are ~885k RLE1 symbols, 51x
    z = bytes(43 << 20)
    c = bz2.compress(z, 9)
    rc, out = threads(bh, c, 4)
    assert rc == 0 and out == z
    assert len(chain(bh, c)) == 1


def test_concatenated_streams_of_different_levels(bh):
    a, b, c = text(250000, 7), bytes(range(256)) * 900, text(1300000, 8)
    z = bz2.compress(a, 1) + bz2.compress(b, 5) + bz2.compress(c, 9)
    assert bz2.decompress(z) == a + b + c
    assert both(bh, z) == (0, a + b + c)
    assert both(bh, bz2.compress(b"", 3) + bz2.compress(a, 2)) == (0, a)


def test_block_starts_are_among_the_candidates_at_odd_bits(bh):
    d = text(6 << 20, 9)
    z = bz2.compress(d, 1)
    starts = chain(bh, z)
    assert len(starts) >= 50
    total, cand = candidates(bh, z)
    assert total == len(cand) and set(starts) <= set(cand)
    assert any(s % 8 for s in starts), "every block start byte aligned: the bit scan is not exercised"
    for s in cand:  # every candidate is the magic at that bit
        word = int.from_bytes(z[s // 8: s // 8 + 8].ljust(8, b"\0"), "big")
        assert (word << (s % 8) & (1 << 64) - 1) >> 16 == BLOCK_MAGIC


def test_linking_with_false_candidates(bh):
    d = text(3 << 20, 10)
    z = bz2.compress(d, 2)
    starts = chain(bh, z)
    r = random.Random(12)
    false = sorted(set(r.randrange(32, len(z) * 8 - 64) for _ in range(300)) - set(starts))
    for cand in (sorted(starts + false), sorted(starts[::2] + false[:40]), []):
        rc, out = link(bh, z, cand, r.choice([2, 4]))
        assert rc == 0 and out == d


def _set_bits(z, bit, width, value):
    b = bytearray(z)
    for k in range(width):
        pos = bit + k
        v = (value >> (width - 1 - k)) & 1
        if v:
            b[pos // 8] |= 0x80 >> (pos % 8)
        else:
            b[pos // 8] &= ~(0x80 >> (pos % 8)) & 0xff
    return bytes(b)


def _eos_bit(z):
    v = int.from_bytes(z, "big")
    for bit in range(len(z) * 8 - 80, len(z) * 8 - 96, -1):
        if (v >> (len(z) * 8 - bit - 48)) & ((1 << 48) - 1) == 0x177245385090:
            return bit
    raise AssertionError("no end-of-stream magic")


def test_malformed_streams_are_eformat(bh):
    d = text(300000, 13)
    z = bz2.compress(d, 9)
    assert both(bh, b"")[0] == EFORMAT
    for cut in (1, 3, 4, 5, 10, 20, 100, len(z) // 2, len(z) - 11, len(z) - 10, len(z) - 5, len(z) - 1):
        assert both(bh, z[:cut])[0] == EFORMAT, cut
    assert both(bh, b"BZh0" + z[4:])[0] == EFORMAT
    assert both(bh, b"BZhA" + z[4:])[0] == EFORMAT
    assert both(bh, z + b"junk")[0] == EFORMAT
    assert both(bh, z + b"\0")[0] == EFORMAT
    assert both(bh, z + b"BZh")[0] == EFORMAT
    # the first block starts at bit 32: magic 48, CRC 32, randomised 1, origPtr 24
    rand = _set_bits(z, 32 + 48 + 32, 1, 1)
    assert both(bh, rand)[0] == EFORMAT
    assert both(bh, _set_bits(z, 32 + 48 + 33, 24, 300000))[0] == EFORMAT  # origPtr >= the block's symbol count
    assert both(bh, _set_bits(z, 32 + 48, 32, 0x12345678))[0] == EFORMAT   # block CRC
    eos = _eos_bit(z)  # combined CRC: the 32 bits after the end-of-stream magic
    assert both(bh, _set_bits(z, eos + 48, 32, 0x12345678))[0] == EFORMAT
    # a block longer than its level allows: a level-9 block relabelled as level 1
    assert both(bh, b"BZh1" + z[4:])[0] == EFORMAT


def test_single_bit_flips_are_caught(bh):
    d = text(120000, 14)
    z = bz2.compress(d, 9)
    r = random.Random(15)
    for _ in range(400):
        bit = r.randrange(0, len(z) * 8)
        m = bytearray(z)
        m[bit // 8] ^= 0x80 >> (bit % 8)
        rc, out = both(bh, bytes(m))
        assert rc in (0, EFORMAT)
        if rc == 0:  # (a flip in the padding bits: the stream is still what libbz2 reads)
            assert out == d and bz2.decompress(bytes(m)) == d


def test_planted_magics_past_the_cap(bh):
    d = text(2 << 20, 16)
    z = bz2.compress(d, 1)
    magic = BLOCK_MAGIC.to_bytes(6, "big")
    planted = z + magic * 200000  # more magics than the candidate cap of the whole input
    total, _ = candidates(bh, planted, 16)
    assert total > len(planted) // 32 + 64
    assert both(bh, planted)[0] == EFORMAT
    mid = len(z) // 2
    inside = z[:mid] + magic * 100000 + z[mid:]
    assert both(bh, inside)[0] == EFORMAT
    assert both(bh, z) == (0, d)


def test_crc_is_crc32_bzip2(bh):
    # bzip2's CRC is the MSB-first one: its value for "123456789" is the CRC-32/BZIP2 check value
    assert bh.bh_crc(b"123456789", 9) == 0xFC891918


def test_bzip2_host_code_under_asan_and_ubsan(bh, tmp_path):
    exe = hostbuild.sanitized(["tests/bzip2_host_harness.cpp"], defines=["BH_MAIN"])
    d = text(40000, 17) + bytes(range(256)) * 20 + bytes(3000)
    z = bz2.compress(d[:30000], 1) + bz2.compress(d, 9)
    f = tmp_path / "in.bz2"
    f.write_bytes(z)
    hostbuild.run_sanitized(exe, [f, 3000, 7], timeout=900)
    planted = tmp_path / "planted.bz2"
    planted.write_bytes(z + BLOCK_MAGIC.to_bytes(6, "big") * 5000)
    hostbuild.run_sanitized(exe, [planted, 40, 8], timeout=900)


def run_free(n, seed):
    """n random bytes, each different from the one before: no run, so RLE1 leaves them as they are."""
    rng = np.random.default_rng(seed)
    return (np.cumsum(rng.integers(1, 256, size=n)) % 256).astype(np.uint8).tobytes()


def periodic_unit(size, seed):
    """A run-free unit u whose last byte differs from its first: u * k is run-free and has period exactly |u|."""
    rng = np.random.default_rng(seed)
    while True:
        u = (np.cumsum(rng.integers(1, 256, size=size)) % 256).astype(np.uint8).tobytes()
        if size == 1 or (u[0] != u[-1] and len(set(u)) > 1):
            return u


SAMPLE_NS = (1, 2, 3, 63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097, 99981, 899981)
UNIT_SIZES = (1, 2, 3, 5, 16, 1000)


def block_bwt(L, data, level=9):
    """libbz2's BWT bytes and origPtr of `data`, which must be one block: the symbol stage of bz2.compress's output."""
    z = bz2.compress(data, level)
    bwt = ctypes.create_string_buffer(900000)
    op = ctypes.c_uint32()
    n = L.bh_block_bwt(z, len(z), 32, bwt, ctypes.byref(op))
    assert n > 0 and len(chain(L, z)) == 1, n
    return bwt.raw[:n], op.value


def ibwt_both(L, bwt, op):
    """(the sampled walk's status, its output, its cycle length, the serial walk's output) for (bwt, origPtr)."""
    n = len(bwt)
    a, b, cyc = ctypes.create_string_buffer(n), ctypes.create_string_buffer(n), ctypes.c_uint32()
    rc = L.bh_ibwt_sampled(bwt, n, op, a, ctypes.byref(cyc))
    L.bh_ibwt(bwt, n, op, b)
    return rc, a.raw, cyc.value, b.raw


def orig_ptr_classes(n, op):
    """origPtr itself, 0, n - 1, a multiple of the kernels' sample stride and (where the stride is > 1) no multiple."""
    stride = -(-n // 2048)
    ns = -(-n // stride)
    ops = {op, 0, n - 1, stride * (ns // 2)}
    if stride > 1:
        ops |= {stride * (ns // 3) + 1, n - 2 if (n - 2) % stride else n - 3}
    return sorted(o for o in ops if 0 <= o < n)


def check_sampled(L, bwt, op, cycle=None):
    for o in orig_ptr_classes(len(bwt), op):
        rc, got, cyc, want = ibwt_both(L, bwt, o)
        assert rc == 0 and got == want, (len(bwt), o, cyc)
        if cycle is not None:
            assert cyc == cycle, (len(bwt), o, cyc, cycle)


def test_sampled_ibwt_on_primitive_blocks(bh):
    for n in SAMPLE_NS:
        data = run_free(n, n)
        bwt, op = block_bwt(bh, data)
        assert len(bwt) == n
        rc, got, cyc, want = ibwt_both(bh, bwt, op)
        assert rc == 0 and got == want == data and cyc == n, (n, cyc)
        check_sampled(bh, bwt, op, n)


def test_sampled_ibwt_on_periodic_blocks(bh):
    """u^k after RLE1: the permutation has k cycles of |u|, and the n steps from origPtr go round one of them k times.
    The kernels once required one cycle through every sample and refused every such block."""
    seen = set()
    for size in UNIT_SIZES:
        for n in SAMPLE_NS:  # at each n where k is an integer, else at the largest multiple of |u| below it
            n -= n % size
            if n // size < 2 or (size, n) in seen:
                continue
            u = periodic_unit(size, size * 7 + n)
            data = u * (n // size)
            if size == 1:  # a run: its RLE1 form is no longer u^k, but a block of one byte value is its own BWT
                bwt, op = data, n // 3
            else:
                bwt, op = block_bwt(bh, data)
                assert len(bwt) == n
            rc, got, cyc, want = ibwt_both(bh, bwt, op)
            assert rc == 0 and got == want == data and cyc == size, (size, n, cyc)
            check_sampled(bh, bwt, op, size)
            seen.add((size, n))
    assert len(seen) >= 45


def test_sampled_ibwt_on_arbitrary_permutations(bh):
    """(bwt, origPtr) pairs that are the BWT of nothing: several cycles of unequal length, L need not divide n.  The
    output is still the n-step walk (a corrupt block: its CRC refuses it)."""
    r = random.Random(21)
    rng = np.random.default_rng(22)
    short = 0
    for it in range(400):
        n = r.choice([r.randrange(1, 70), r.randrange(1, 5000), r.randrange(2040, 4200), r.randrange(1, 300000)])
        if it < 4:
            n = (899981, 900000, 99981, 4097)[it]
        bwt = rng.integers(0, r.choice([1, 2, 3, 4, 17, 256]), size=n, dtype=np.uint8).tobytes()
        op = r.choice([0, n - 1, r.randrange(n)])
        rc, got, cyc, want = ibwt_both(bh, bwt, op)
        assert rc == 0 and got == want and 1 <= cyc <= n, (n, op, cyc)
        short += cyc < n and n % cyc != 0
    assert short >= 50, short  # many cycles whose length does not divide n


def periodic_streams():
    """Streams of one block each that is exactly periodic after RLE1 (tests/test_gpu_bzip2_edges.py runs them on the
    kernels): (data, level)."""
    out = []
    for k in (2, 3):
        for v in (0, 0x41, 0xff):
            out.append((bytes([v]) * k, 9))
    for m in (2, 3, 409, 3529, 179996):  # RLE1: b"\0\0\0\0\xfb" * m
        out.append((bytes(255 * m), 9))
    for size in (2, 3, 16, 1000):
        u = periodic_unit(size, size)
        for cap in (2048, 4096, 99981, 899981):
            out.append((u * (cap // size), 1 if cap <= 99981 else 9))
    return out


def test_periodic_blocks_on_the_host(bh):
    for data, lv in periodic_streams():
        z = bz2.compress(data, lv)
        assert len(chain(bh, z)) == 1, len(data)
        assert both(bh, z) == (0, data), len(data)
