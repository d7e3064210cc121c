"""data.tar.xz on the CPU: the .xz container and the LZMA2 / LZMA decoder (snappy_amd/csrc/xz_core.h, xz_host.cpp)
compiled for the host (tests/xz_host_harness.cpp) and checked against liblzma through Python's lzma -- every good file
of tests/xz_cases.py byte for byte, every bad one refused, every unsupported one handed back -- with the harness's
histogram showing that each edge shape really occurred; the kernel's wave-copy index arithmetic run lane by lane; the
CRC-64 core against the bitwise routine; and the bad cases once more under ASan/UBSan.  The GPU kernel that runs the same
header is checked in tests/test_gpu_unxz.py and tests/test_gpu_xz_edges.py."""
import ctypes
import functools
import hashlib
import os
import random

import pytest

import xz_cases as X
import hostbuild
from conftest import ROOT

HARNESS = os.path.join(ROOT, "tests", "xz_host_harness.cpp")
EINVAL, EFORMAT = -1, -9
# the histogram's layout (xz_host_harness.cpp)
H_LIT, H_MATCHED_LIT, H_MATCH, H_REP, H_SHORT_REP, H_DIST_ALL, H_DIST_DICT, H_COPY, H_CTL = 0, 1, 2, 3, 7, 8, 9, 10, 26
H_LC, H_LP, H_PB, H_CHUNK_1, H_CHUNK_2M, H_CHUNK_BIG, H_N = 282, 287, 292, 297, 298, 299, 300
POLY = 0xC96C5795D7870F42


@functools.lru_cache(maxsize=None)
def load_xh():
    """tests/xz_host_harness.cpp, loaded once a process with every prototype (it keeps no state between calls)."""
    L = hostbuild.shared(HARNESS)
    P = ctypes.POINTER
    L.xh_decode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint, P(ctypes.c_size_t), P(ctypes.c_int)]
    L.xh_decode.restype = ctypes.c_void_p
    L.xh_free.argtypes = [ctypes.c_void_p]
    L.xh_hist.argtypes = [ctypes.c_char_p, ctypes.c_size_t, P(ctypes.c_uint64)]
    L.xh_copy_check.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    L.xh_copy_check.restype = ctypes.c_uint64
    for f, a in (("xh_crc64", [ctypes.c_char_p, ctypes.c_size_t]), ("xh_crc64_cut", [ctypes.c_char_p, ctypes.c_size_t]),
                 ("xh_crc64_combine", [ctypes.c_uint64] * 3), ("xh_crc64_xpow8", [ctypes.c_uint64]), ("xh_crc64_table", [ctypes.c_uint32] * 2)):
        getattr(L, f).argtypes = a
        getattr(L, f).restype = ctypes.c_uint64
    L.xh_sha256.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    return L


@pytest.fixture(scope="module")
def xh():
    return load_xh()


def decode(L, z, threads=4):
    n, rc = ctypes.c_size_t(), ctypes.c_int()
    p = L.xh_decode(z, len(z), threads, ctypes.byref(n), ctypes.byref(rc))
    b = ctypes.string_at(p, n.value)
    L.xh_free(p)
    return rc.value, b


def hist(L, z):
    h = (ctypes.c_uint64 * H_N)()
    assert L.xh_hist(z, len(z), h) == 0
    return list(h)


def test_good_files_decode_to_liblzmas_bytes(xh):
    for name, z, plain in X.good_cases():
        for t in (1, 4):
            rc, b = decode(xh, z, t)
            assert rc == 0 and b == plain, (name, t, rc)


def test_bad_files_are_refused(xh):
    for name, z, _ in X.bad_cases():
        assert decode(xh, z) == (EFORMAT, b""), name
    assert decode(xh, b"") == (EFORMAT, b"")


def test_unsupported_files_are_einval(xh):
    for name, z in X.unsupported_cases():
        assert decode(xh, z)[0] == EINVAL, name


def test_every_edge_shape_occurred(xh):
    """The builders only ask liblzma's encoder for the shapes; this shows that it produced them."""
    h = {name: hist(xh, z) for name, z, _ in X.edge_cases()}
    for di, d in enumerate(X.COPY_DISTS):
        for li, ln in enumerate(X.COPY_LENS):
            g = h["copy_d%d_l%d" % (d, ln)]
            assert g[H_COPY + 4 * di + li] >= 1, (d, ln, g[H_COPY:H_COPY + 16])
    assert h["copy_d64_l64"][H_DIST_ALL] >= 1                      # a distance equal to the bytes produced so far
    assert h["dist_is_dict_size"][H_DIST_DICT] >= 1                # and one equal to the dictionary size
    r = h["reps"]
    assert all(r[H_REP + k] >= 1 for k in range(4)) and r[H_SHORT_REP] >= 1 and r[H_MATCHED_LIT] >= 1 and r[H_MATCH] >= 1 and r[H_LIT] >= 1
    assert h["lc4_lp0"][H_LC + 4] and h["lc4_lp0"][H_LP + 0] and h["lc0_lp4"][H_LC + 0] and h["lc0_lp4"][H_LP + 4]
    assert h["pb0"][H_PB + 0] and h["pb4"][H_PB + 4]
    assert h["one_byte"][H_CHUNK_1] == 1
    # liblzma's encoder closes a chunk a match length short of 2 MiB: the largest chunk it writes, not one of exactly 2 MiB
    assert h["chunk_near_2mib"][H_CHUNK_BIG] >= 1
    assert h["chunk_2mib"][H_CHUNK_2M] >= 1  # exactly 2 MiB, from tests/xz_cases.py's own range encoder
    u = h["uncompressed_chunks"]
    assert u[H_CTL + 1] == 1 and u[H_CTL + 2] >= 1
    assert sum(h["chunks_continue"][H_CTL + 0x80:H_CTL + 0xA0]) >= 1  # chunks that continue the probabilities
    e0 = h["e0_mid_block"]
    assert sum(e0[H_CTL + 0xE0:H_CTL + 0x100]) == 2 and len([k for k in range(5) if e0[H_LC + k]]) == 2
    assert sum(h["c0_mid_block"][H_CTL + 0xC0:H_CTL + 0xE0]) == 1
    assert sum(h["a0_mid_block"][H_CTL + 0xA0:H_CTL + 0xC0]) == 1
    assert h["blocks_300"][H_CTL + 0] == 300


def test_wave_copy_arithmetic_lane_by_lane(xh):
    assert xh.xh_copy_check(130, 273) == 0


def _raw(msg):
    """The raw remainder (init 0, no final xor), bit by bit."""
    c = 0
    for x in msg:
        c ^= x
        for _ in range(8):
            c = (c >> 1) ^ (POLY if c & 1 else 0)
    return c


def _mul(p, q):
    out = 0
    for i in range(63, -1, -1):
        if p >> i & 1:
            out ^= q
        q = (q >> 1) ^ (POLY if q & 1 else 0)
    return out


def _xpow8(n):
    res, base = 1 << 63, 1 << 55
    while n:
        if n & 1:
            res = _mul(res, base)
        base = _mul(base, base)
        n >>= 1
    return res


def test_crc64_core_against_the_bitwise_routine(xh):
    r = random.Random(7)
    for n in list(range(0, 70)) + [255, 256, 257, 4095, 65535, 65536, 65537, 200001]:
        data = r.randbytes(n)
        want = X.crc64(data) if n < 5000 else X.crc64_fast(data)
        assert xh.xh_crc64(data, n) == want, n          # slice-by-8
        assert xh.xh_crc64_cut(data, n) == want, n      # the kernels' cut from the range's end, folded
    a, b = r.randbytes(1000), r.randbytes(777)
    assert xh.xh_crc64_combine(X.crc64(a), X.crc64(b), len(b)) == X.crc64(a + b)
    assert xh.xh_crc64_combine(X.crc64(a), X.crc64(b""), 0) == X.crc64(a)
    for k in (0, 1, 7):  # table k, entry b: the raw remainder of byte b followed by k zero bytes
        for byte in (1, 0x80, 0xFF):
            assert xh.xh_crc64_table(k, byte) == _raw(bytes([byte]) + bytes(k)), (k, byte)
    assert xh.xh_crc64_xpow8(0) == 1 << 63
    assert xh.xh_crc64_xpow8(3) == _xpow8(3) == 1 << 39  # x^24, below the polynomial's degree
    assert xh.xh_crc64_xpow8((1 << 32) + 3) == _xpow8((1 << 32) + 3)


def test_sha256(xh):
    for n in (0, 1, 55, 56, 63, 64, 65, 119, 120, 1000):
        data = X.rnd(n, n)
        out = ctypes.create_string_buffer(32)
        xh.xh_sha256(data, n, out)
        assert out.raw == hashlib.sha256(data).digest(), n


def test_xz_host_code_under_asan_and_ubsan(tmp_path):
    """Host code only: every bad and unsupported file and the small good ones through an instrumented build, each from a
    heap buffer of exactly its size."""
    main = tmp_path / "main.cpp"
    main.write_text('#include "%s"\n#include <stdio.h>\nint main(int argc, char** argv) { for (int i = 1; i < argc; ++i) { FILE* f = fopen(argv[i], "rb"); '
                    'std::vector<uint8_t> z(1 << 22); size_t n = fread(z.data(), 1, z.size(), f); fclose(f); z.resize(n); std::vector<uint8_t> exact(z); '
                    'size_t ol; int rc; void* p = xh_decode(exact.data(), exact.size(), 2, &ol, &rc); xh_free(p); printf("%%d\\n", rc); } return 0; }\n' % HARNESS)
    exe = hostbuild.sanitized([main])
    files, want = [], []
    cases = [(n, z, EFORMAT) for n, z, _ in X.bad_cases()] + [(n, z, EINVAL) for n, z in X.unsupported_cases()]
    cases += [(n, z, 0) for n, z, _ in X.good_cases() if len(z) < 100000]
    for i, (name, z, rc) in enumerate(cases):
        p = tmp_path / ("c%03d" % i)
        p.write_bytes(z)
        files.append(str(p))
        want.append(rc)
    out = hostbuild.run_sanitized(exe, files)
    assert [int(x) for x in out.stdout.split()] == want
