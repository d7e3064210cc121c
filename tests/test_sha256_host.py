"""sha256_core.h on the CPU (tests/sha256_host_harness.cpp), against hashlib.sha256: the core at every length where the
tail takes one block or two, the kernel's lane routine run serially -- the aligned 16-byte fetch, the funnel shift and the
tail at every start alignment, with every fetched word counted -- and the .xz writer's host model with each Check, read by
liblzma.  The kernel itself: tests/test_gpu_sha256_edges.py; both sides of the library: tests/test_gpu_xz_sha256.py."""
import ctypes
import functools
import hashlib
import lzma
import random

import pytest

import hostbuild

CHECKS = {0: 0, 1: 4, 4: 8, 10: 32}  # Check id -> bytes of the field


@functools.lru_cache(maxsize=None)
def load_sha(opt="-O2"):
    """tests/sha256_host_harness.cpp, loaded once a process with every prototype (it keeps no state between calls).
    opt: tools/sha256_bench.py times it at -O3."""
    L = hostbuild.shared("tests/sha256_host_harness.cpp", opt)
    L.sh_sha256.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p]
    L.sh_sha256.restype = None
    L.sh_lane.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64]
    L.sh_lane.restype = ctypes.c_uint64
    L.sh_blocks.argtypes = [ctypes.c_uint64]
    L.sh_blocks.restype = ctypes.c_uint64
    for f in (L.sh_block_bytes, L.sh_load_bytes, L.sh_step_bytes, L.sh_tile_row_bytes):
        f.restype = ctypes.c_uint32
    L.sh_xz_encode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t),
                               ctypes.POINTER(ctypes.c_int)]
    L.sh_xz_encode.restype = ctypes.c_void_p
    L.sh_free.argtypes = [ctypes.c_void_p]
    return L


def model_xz(L, data, block_size, check=None):
    """The host model's file for `data` (check None: through the signature that names no Check); None if refused."""
    n, rc = ctypes.c_size_t(), ctypes.c_int()
    p = L.sh_xz_encode(data, len(data), block_size, check or 0, check is not None, ctypes.byref(n), ctypes.byref(rc))
    try:
        return None if rc.value else ctypes.string_at(p, n.value)
    finally:
        L.sh_free(p)


@pytest.fixture(scope="module")
def sh():
    return load_sha()


@pytest.fixture(scope="module")
def buf():
    return random.Random(256).randbytes(65537 + 64)


def test_core_lengths(sh, buf):
    """0..300 holds 55 / 56, 63 / 64 / 65 and 119 / 120: where the tail takes one block or two."""
    out = ctypes.create_string_buffer(32)
    for n in list(range(301)) + [65535, 65536, 65537]:
        sh.sh_sha256(buf[:n], n, out)
        assert out.raw == hashlib.sha256(buf[:n]).digest(), n
        assert sh.sh_blocks(n) == (n + 9 + 63) // 64


def test_lane_alignments_and_fetches(sh, buf):
    """The lane routine at every start alignment and the lengths 0..130: the digest, and which aligned words it read."""
    assert (sh.sh_block_bytes(), sh.sh_load_bytes()) == (64, 16)
    cap = 16
    raw = ctypes.create_string_buffer(cap * 16 + 16)
    base = (ctypes.addressof(raw) + 15) & ~15  # the harness's words are aligned as the kernel's are
    ctypes.memmove(base, buf, cap * 16)
    out = ctypes.create_string_buffer(32)
    for a in range(16):
        for n in range(131):
            fetched = (ctypes.c_uint32 * cap)()
            outside = sh.sh_lane(base, a, n, out, fetched, cap)
            assert out.raw == hashlib.sha256(buf[a:a + n]).digest(), (a, n)
            assert outside == 0, (a, n)
            want = [1 if n and 16 * j < a + n else 0 for j in range(cap)]  # (a < 16: word 0 overlaps whenever n > 0)
            assert list(fetched) == want, (a, n)


def test_lane_long_range(sh, buf):
    out = ctypes.create_string_buffer(32)
    cap = 65536 // 16 + 2
    raw = ctypes.create_string_buffer(cap * 16 + 16)
    base = (ctypes.addressof(raw) + 15) & ~15
    ctypes.memmove(base, buf, min(len(buf), cap * 16))
    for a, n in ((0, 65536), (5, 65535), (15, 65537 - 15), (16 + 3, 4097)):
        fetched = (ctypes.c_uint32 * cap)()
        assert sh.sh_lane(base, a, n, out, fetched, cap) == 0
        assert out.raw == hashlib.sha256(buf[a:a + n]).digest(), (a, n)
        assert max(fetched) == 1


@pytest.fixture(scope="module")
def data200k():
    rnd = random.Random(19)
    words = [rnd.randbytes(rnd.randrange(3, 12)) for _ in range(300)]
    out = bytearray()
    while len(out) < 200_000:
        out += rnd.choice(words)
    return bytes(out[:200_000])


@pytest.mark.parametrize("check", sorted(CHECKS))
def test_container_with_each_check(sh, data200k, check):
    xz = model_xz(sh, data200k, 65536, check)
    assert xz is not None
    assert lzma.decompress(xz) == data200k  # (liblzma verifies every Check it knows: all four)
    assert xz[6:8] == bytes([0, check]) and xz[-4:-2] == bytes([0, check])  # the Stream flags of header and footer
    if check == 4:
        assert model_xz(sh, data200k, 65536, None) == xz
    if check == 10:
        # the last Block's Check field ends where the Index begins: the Index is 4-byte aligned and its size is in the footer
        index_size = (int.from_bytes(xz[-8:-4], "little") + 1) * 4
        last = len(xz) - 12 - index_size - 1
        bad = bytearray(xz)
        bad[last] ^= 0x10
        with pytest.raises(lzma.LZMAError):
            lzma.decompress(bytes(bad))
        bad = bytearray(xz)
        bad[last - 31] ^= 0x01  # the field's first byte
        with pytest.raises(lzma.LZMAError):
            lzma.decompress(bytes(bad))


def test_container_refuses_other_checks(sh, data200k):
    for check in (2, 3, 11, 15):
        assert model_xz(sh, data200k[:100], 65536, check) is None
