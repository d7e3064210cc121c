"""crc_core.h on the CPU (tests/crc_host_harness.cpp): both CRC-32 flavours against zlib.crc32 and a table CRC held
against libbz2 (tests/crc_oracle.py), combine at every split point and with lengths of 0 and of more than 2^32, and the
kernels' cut of a range into tiles and lane slices run serially.  The kernels themselves: tests/test_gpu_crc_edges.py."""
import ctypes
import functools
import random
import zlib

import pytest

import crc_oracle
import hostbuild
from crc_oracle import BZIP2, GZIP

KINDS = [GZIP, BZIP2]


@functools.lru_cache(maxsize=None)
def load_ch():
    """tests/crc_host_harness.cpp, loaded once a process with every prototype (it keeps no state between calls)."""
    L = hostbuild.shared("tests/crc_host_harness.cpp")
    for f in (L.ch_crc, L.ch_tiled):
        f.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64]
        f.restype = ctypes.c_uint32
    L.ch_combine.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]
    L.ch_combine.restype = ctypes.c_uint32
    L.ch_slice.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    L.ch_slice.restype = None
    L.ch_tiles.argtypes = [ctypes.c_uint64]
    L.ch_tiles.restype = ctypes.c_uint64
    L.ch_tile_bytes.restype = ctypes.c_uint32
    L.ch_slice_bytes.restype = ctypes.c_uint32
    return L


@pytest.fixture(scope="module")
def ch():
    return load_ch()


@pytest.fixture(scope="module")
def buf():
    return random.Random(11).randbytes((3 << 16) + 64)


def test_bz_oracle_is_libbz2s():
    crc_oracle.check_bz_oracle()


@pytest.mark.parametrize("kind", KINDS)
def test_lengths(ch, buf, kind):
    for n in list(range(41)) + [65535, 65536, 65537]:
        for start in (0, 1, 7):  # the 16-byte loads begin where the ADDRESS allows: shift it
            d = buf[start:start + n]
            assert ch.ch_crc(kind, d, n) == crc_oracle.crc(kind, d), (kind, n, start)
    for fill in (b"\0", b"\xff"):
        d = fill * 1000
        assert ch.ch_crc(kind, d, len(d)) == crc_oracle.crc(kind, d)


@pytest.mark.parametrize("kind", KINDS)
def test_combine_every_split(ch, buf, kind):
    d = buf[:100]
    want = crc_oracle.crc(kind, d)
    for k in range(101):
        a, b = crc_oracle.crc(kind, d[:k]), crc_oracle.crc(kind, d[k:])
        assert ch.ch_combine(kind, a, b, 100 - k) == want, k
    a = crc_oracle.crc(kind, d)
    assert ch.ch_combine(kind, a, 0, 0) == a  # len_b == 0: B is empty, its CRC is 0


def _crc_then_zeros(kind, head, nzeros):
    """The CRC of head followed by nzeros zero bytes, a chunk at a time."""
    if kind == GZIP:
        c = zlib.crc32(head)
        chunk = bytes(1 << 24)
        left = nzeros
        while left:
            k = min(left, len(chunk))
            c = zlib.crc32(chunk[:k] if k < len(chunk) else chunk, c)
            left -= k
        return c & 0xFFFFFFFF
    # bzip2's flavour: the finished CRC c stands for the register ~c; n zero bytes multiply it by x^(8n)
    return crc_oracle._zeros(crc_oracle.bz_crc(head) ^ 0xFFFFFFFF, nzeros) ^ 0xFFFFFFFF


@pytest.mark.parametrize("kind", KINDS)
def test_combine_past_4gib(ch, buf, kind):
    n = (1 << 32) + 3
    head = buf[:100]
    a = crc_oracle.crc(kind, head)
    if kind == GZIP:
        # the CRC of n zero bytes, and of head + n zero bytes, both by zlib over chunks
        zeros = _crc_then_zeros(kind, b"", n)
        want = _crc_then_zeros(kind, head, n)
    else:
        # the oracle's zero-run step is first held against its own byte loop on a length the loop can walk
        assert crc_oracle._zeros(crc_oracle.bz_crc(head) ^ 0xFFFFFFFF, 5000) ^ 0xFFFFFFFF == crc_oracle.bz_crc(head + bytes(5000))
        zeros = _crc_then_zeros(kind, b"", n)
        want = _crc_then_zeros(kind, head, n)
    assert ch.ch_combine(kind, a, zeros, n) == want
    assert ch.ch_combine(kind, 0, zeros, n) == zeros  # A empty


def test_cut_covers_every_byte_once(ch):
    tile, sl = ch.ch_tile_bytes(), ch.ch_slice_bytes()
    lanes = tile // sl
    lo, hi = ctypes.c_uint64(), ctypes.c_uint64()
    for n in (1, sl - 1, sl, sl + 1, tile - 1, tile, tile + 1, 2 * tile + 5):
        nt = ch.ch_tiles(n)
        assert nt == (n + tile - 1) // tile
        at = 0
        for k in range(nt - 1, -1, -1):  # tile nt - 1 (counted from the end) is the range's first
            for lane in range(lanes):
                ch.ch_slice(n, k, lane, ctypes.byref(lo), ctypes.byref(hi))
                if hi.value > lo.value:
                    assert lo.value == at and hi.value - lo.value <= sl, (n, k, lane)
                    at = hi.value
        assert at == n
    assert ch.ch_tiles(0) == 0


@pytest.mark.parametrize("kind", KINDS)
def test_lane_and_tile_emulation(ch, buf, kind):
    tile, sl = ch.ch_tile_bytes(), ch.ch_slice_bytes()
    for n in (0, 1, sl - 1, sl, sl + 1, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1, 3 * tile + 5):
        for start in (0, 3):
            d = buf[start:start + n]
            assert ch.ch_tiled(kind, d, n) == crc_oracle.crc(kind, d), (kind, n, start)
