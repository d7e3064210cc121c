"""snappy_amd/csrc/sha512_core.h (the block + padding logic every HIP kernel
shares) compiled as host C++ and checked against the oracle.  CPU only; the
device build of the same header is checked by the -m gpu parity tests."""
import ctypes
import functools
import os

import pytest

import hostbuild
from conftest import ROOT


H8 = ctypes.c_uint64 * 8


@functools.lru_cache(maxsize=None)
def load_core():
    """tests/core_host_harness.cpp, loaded once a process with every prototype (it keeps no state between calls)."""
    L = hostbuild.shared("tests/core_host_harness.cpp")
    L.core_sha512.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p]
    L.core_sha512.restype = None
    L.core_segment.argtypes = [H8, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int]
    L.core_segment.restype = None
    L.hostsha_resume_final.argtypes = [H8, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p]
    L.hostsha_resume_final.restype = None
    L.hostsha_buffer.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p]
    L.hostsha_buffer.restype = None
    L.hostsha_variants.argtypes = []
    L.hostsha_blocks_variant.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    L.hostsha_blocks_variant.restype = None
    L.hostsha_file.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p]
    L.hostsha_x8_available.argtypes = []
    L.hostsha_many.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint64,
                               ctypes.c_uint, ctypes.c_uint64, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64)]
    return L


@pytest.fixture(scope="module")
def core():
    L = load_core()

    def f(data, split=0):
        out = ctypes.create_string_buffer(64)
        L.core_sha512(data, len(data), split, out)
        return out.raw
    return f


def test_every_tail_length(core, oracle):
    rnd = os.urandom(1024)
    for n in range(0, 520):
        assert core(rnd[:n]) == oracle.sha512(rnd[:n]), n


def test_segment_carry(core, oracle):
    rnd = os.urandom(5000)
    for n in (256, 257, 1000, 4096, 4999, 5000):
        for split in (128, 256, 1024):
            if split < n:
                assert core(rnd[:n], split) == oracle.sha512(rnd[:n]), (n, split)


def test_round_constants_from_first_principles():
    """K512 / IV512 in sha512_core.h against cube/square roots of the primes (FIPS 180-4 sec. 4.2.3, 5.3.5)."""
    import re
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from gen_sha512_constants import constants
    K, IV = constants()
    text = open(os.path.join(ROOT, "snappy_amd", "csrc", "sha512_core.h")).read()
    body = text[text.index("#define SNAPHASH_K512_LIST"):text.index("static constexpr uint64_t K512")]
    got = [int(x, 16) for x in re.findall(r"0x([0-9a-f]{16})ULL", body)]
    assert got == K
    iv = text[text.index("IV512[8] = {"):]
    assert [int(x, 16) for x in re.findall(r"0x([0-9a-f]{16})ULL", iv[:iv.index("};")])] == IV


def test_plain_python_reference_vs_hashlib():
    """tests/sha512_ref.py, which the tests below and tests/test_gpu_sha512_edges.py compare with, against hashlib.sha512:
    every length 0..300, and a 753-byte message cut at every block boundary, the chaining value carried over the cut."""
    import hashlib
    import sha512_ref as ref
    rnd = os.urandom(753)
    for n in range(301):
        assert ref.digest(ref.segment(ref.IV, rnd[:n], 0, True)) == hashlib.sha512(rnd[:n]).digest(), n
    for cut in range(0, 753, 128):
        H = ref.segment(ref.IV, rnd[:cut], 0, False)
        assert ref.digest(ref.segment(H, rnd[cut:], cut, True)) == hashlib.sha512(rnd).digest(), cut
    for cut in range(128, 753, 128):  # and at two of them
        H = ref.segment(ref.segment(ref.IV, rnd[:128], 0, False), rnd[128:cut], 128, False)
        assert ref.digest(ref.segment(H, rnd[cut:], cut, True)) == hashlib.sha512(rnd).digest(), cut


# byte counts a stream has behind it when a segment starts: none, a block, around the 2^32 bits and the 2^32 bytes of a
# 32-bit counter, 5 GiB, the longest resident segment, around 2^61 (where the bit length enters its high word) and the end
# of the 64-bit counter -- the last four no caller reaches, Job.total_prev holds them all the same
TOTAL_PREV = [0, 128, (1 << 29) - 128, 1 << 29, (1 << 32) - 128, 1 << 32, (1 << 32) + 128, 5 << 30, (1 << 35) - 128,
              (1 << 61) - 128, 1 << 61, (1 << 61) + (1 << 32), (1 << 64) - 256]
TAIL_BYTES = [0, 5, 111, 112, 127, 128, 300]


def test_segment_from_any_state_and_byte_count(tmp_path):
    """run_segment (sha512_core.h as a kernel lane walks it) and host_sha512_resume + update + final, each from a random
    chaining value and every byte count of TOTAL_PREV, over every tail of TAIL_BYTES, final: the plain-Python reference's
    digest.  The two length words of the padding are what this is about."""
    import random
    import sha512_ref as ref
    L = load_core()
    rng = random.Random(512)
    out = ctypes.create_string_buffer(64)
    for total_prev in TOTAL_PREV:
        for n in TAIL_BYTES:
            H0 = [rng.getrandbits(64) for _ in range(8)]
            data = rng.randbytes(n)
            want = ref.digest(ref.segment(H0, data, total_prev, True))
            H = H8(*H0)
            L.core_segment(H, data, n, total_prev, 1)
            assert ref.digest(list(H)) == want, ("run_segment", total_prev, n)
            L.hostsha_resume_final(H8(*H0), total_prev, data, n, out)
            assert out.raw == want, ("host_sha512_resume", total_prev, n)
            if n % 128 == 0:  # not final: the byte count plays no part
                H = H8(*H0)
                L.core_segment(H, data, n, total_prev, 0)
                assert list(H) == ref.segment(H0, data, total_prev, False), ("run_segment, not final", total_prev, n)


def test_host_sha512_of_the_hybrid_scheduler(core, tmp_path_factory):
    """snappy_amd/csrc/hostsha.cpp (the library's own host SHA-512, used only when host_threads > 0):
    every tail length, resumed mid-stream from a chaining value, and the file reader's size check."""
    import hashlib
    L = load_core()
    rnd = os.urandom(3000)
    out = ctypes.create_string_buffer(64)
    for n in list(range(0, 300)) + [1000, 2047, 2048, 2049, 3000]:
        for split in (0, 128, 256, 1024):
            L.hostsha_buffer(rnd[:n], n, split, out)
            assert out.raw == hashlib.sha512(rnd[:n]).digest(), (n, split)
    # every spelling of the block function this CPU can run agrees with the portable one, block count by block count
    data = os.urandom(128 * 9)
    for nblocks in range(0, 10):
        got = []
        for v in range(L.hostsha_variants()):
            H = (ctypes.c_uint64 * 8)()
            L.hostsha_blocks_variant(v, data, nblocks, H)
            got.append(list(H))
        assert all(g == got[0] for g in got), nblocks
    p = tmp_path_factory.mktemp("f") / "blob"
    blob = os.urandom((1 << 20) + 77)
    p.write_bytes(blob)
    assert L.hostsha_file(str(p).encode(), len(blob), out) == 0 and out.raw == hashlib.sha512(blob).digest()
    import errno
    assert L.hostsha_file(str(p).encode(), len(blob) - 1, out) == errno.EIO  # grew since its size was taken
    assert L.hostsha_file(str(p).encode(), len(blob) + 1, out) == errno.EIO  # shrank
    assert L.hostsha_file(b"/nonexistent/x", 0, out) == errno.ENOENT
    # a stream of 32 MiB or more is read by a second thread, two buffers ahead of the hasher: same digest, same size checks
    big = tmp_path_factory.mktemp("g") / "big"
    data = os.urandom(1 << 20) * 40 + b"tail"
    big.write_bytes(data)
    for _ in range(3):
        assert L.hostsha_file(str(big).encode(), len(data), out) == 0 and out.raw == hashlib.sha512(data).digest()
    assert L.hostsha_file(str(big).encode(), len(data) - 1, out) == errno.EIO
    assert L.hostsha_file(str(big).encode(), len(data) + (1 << 20), out) == errno.EIO


def test_eight_streams_side_by_side_on_one_core(core, tmp_path_factory):
    """snappy_amd/csrc/hostsha_x8.cpp: a thread of the host pool runs up to eight streams at once, a stream per 64-bit lane
    (AVX-512; one at a time elsewhere).  Memory and files mixed, every length class around the block and the 256 KiB chunk,
    lanes that empty and refill at different times, 1..8 lanes, streams that keep the core to themselves -- every digest
    hashlib's; a file that shrank, grew or is not there fails the call with its errno and its index."""
    import errno
    import hashlib
    import random
    import numpy as np
    L = load_core()
    rng = random.Random(31)
    blob = np.random.default_rng(31).integers(0, 256, size=3 << 20, dtype=np.uint8).tobytes()
    d = tmp_path_factory.mktemp("x8files")
    classes = [0, 1, 111, 112, 127, 128, 129, 255, 256, 4095, 65536, (256 << 10) - 1, 256 << 10, (256 << 10) + 1, (256 << 10) + 128, (512 << 10) + 77, 1 << 20]

    serial = [0]

    def run(specs, lanes, alone_from=0):
        n = len(specs)
        ptrs, paths, lens, keep = (ctypes.c_char_p * n)(), (ctypes.c_char_p * n)(), (ctypes.c_uint64 * n)(), []
        for i, (kind, data, claimed) in enumerate(specs):
            lens[i] = len(data) if claimed is None else claimed
            if kind == "mem":
                keep.append(ctypes.create_string_buffer(data, max(len(data), 1)))
                ptrs[i] = ctypes.cast(keep[-1], ctypes.c_char_p)
            else:
                serial[0] += 1
                p = d / ("f%d" % serial[0])
                keep.append(p)
                if kind != "missing":
                    p.write_bytes(data)
                paths[i] = str(p).encode()
        out = ctypes.create_string_buffer(64 * n)
        bad = ctypes.c_int64(-7)
        rc = L.hostsha_many(ptrs, paths, lens, n, lanes, alone_from, out, ctypes.byref(bad))
        return rc, bad.value, [out.raw[64 * i:64 * i + 64] for i in range(n)]

    for trial in range(60):
        n = rng.randrange(1, 24)
        specs = []
        for i in range(n):
            size = rng.choice(classes) if rng.random() < 0.6 else rng.randrange(0, 700000)
            off = rng.randrange(0, len(blob) - size)
            specs.append((rng.choice(["mem", "file"]), blob[off:off + size], None))
        if trial % 3 == 0:
            specs.sort(key=lambda s: -len(s[1]))  # longest first, as the pool hands them out
        rc, bad, digs = run(specs, rng.randrange(1, 9), alone_from=(300000 if trial % 3 == 0 else 0))
        assert rc == 0 and bad == -1
        assert digs == [hashlib.sha512(s[1]).digest() for s in specs], trial
    # the reference's io.Copy reads what is there: a size taken earlier that no longer holds is an error, whichever lane
    base = [("file", blob[:70000], None)] * 5
    for wrong, code in ((("file", blob[:50000], 50001), errno.EIO), (("file", blob[:50000], 49999), errno.EIO),
                        (("file", blob[:300000], 300128), errno.EIO), (("missing", b"", 10), errno.ENOENT)):
        specs = base[:3] + [wrong] + base[3:]
        for lanes in (1, 8):
            rc, bad, _ = run(specs, lanes)
            assert rc == code and bad == 3, (wrong[2], lanes, rc, bad)


def test_eight_streams_under_asan_and_ubsan(tmp_path):
    """tests/asan_hostsha_x8.cpp: the lane scheduler and the AVX-512 block function with every read checked."""
    exe = hostbuild.sanitized(["tests/asan_hostsha_x8.cpp", "snappy_amd/csrc/hostsha.cpp", "snappy_amd/csrc/hostsha_x8.cpp"])
    work = tmp_path / "files"
    work.mkdir()
    assert "asan x8 driver ok" in hostbuild.run_sanitized(exe, [work]).stdout
