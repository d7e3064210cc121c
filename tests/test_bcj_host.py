"""The .xz BCJ filters on the CPU: snappy_amd/csrc/bcj_core.h compiled for the host (tests/bcj_host_harness.cpp) and held
against liblzma through Python's lzma (tests/bcj_cases.py says how) -- the three filters in both directions on every edge
input, the kernels' cut run stretch by stretch against the serial bytes, xz_plan with and without the BCJ chains allowed,
the host decoder over liblzma's files, the producer's host model with each filter, and the same cases under ASan/UBSan in
a program of its own.  The kernels that run the same header are checked in tests/test_gpu_bcj_edges.py, the entry points
in tests/test_gpu_xz_bcj.py."""
import ctypes
import functools
import lzma

import pytest

import bcj_cases as B
import xz_cases as X
import hostbuild

EINVAL, EFORMAT = -1, -9
PLAN_OK, PLAN_FORMAT, PLAN_UNSUPPORTED = 0, 1, 2


@functools.lru_cache(maxsize=None)
def load_bcj():
    """tests/bcj_host_harness.cpp, loaded once a process with every prototype (it keeps no state between calls)."""
    L = hostbuild.shared("tests/bcj_host_harness.cpp")
    P = ctypes.POINTER
    L.bh_block.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32]
    L.bh_block.restype = None
    L.bh_cut.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
    L.bh_cut.restype = None
    L.bh_plan.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, P(ctypes.c_uint64), P(ctypes.c_uint32), P(ctypes.c_uint32), ctypes.c_size_t,
                          ctypes.c_char_p]
    L.bh_decode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint, ctypes.c_int, P(ctypes.c_size_t), P(ctypes.c_int)]
    L.bh_decode.restype = ctypes.c_void_p
    L.bh_encode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32, P(ctypes.c_size_t), P(ctypes.c_int)]
    L.bh_encode.restype = ctypes.c_void_p
    L.bh_free.argtypes = [ctypes.c_void_p]
    return L


@pytest.fixture(scope="module")
def bh():
    return load_bcj()


def block(L, filt, encode, data, start=0):
    buf = ctypes.create_string_buffer(bytes(data), len(data))
    L.bh_block(filt, int(encode), buf, len(data), start)
    return buf.raw


def cut(L, filt, encode, data, start, stretch, order):
    buf = ctypes.create_string_buffer(bytes(data), len(data))
    points = (ctypes.c_uint32 * (len(data) // stretch + 1))()
    L.bh_cut(filt, int(encode), buf, len(data), start, stretch, order, points)
    return buf.raw


def plan(L, z, allow):
    n = ctypes.c_uint64()
    bcj, starts = (ctypes.c_uint32 * 16)(), (ctypes.c_uint32 * 16)()
    why = ctypes.create_string_buffer(128)
    rc = L.bh_plan(z, len(z), int(allow), ctypes.byref(n), bcj, starts, 16, why)
    k = min(n.value, 16)
    return rc, list(bcj)[:k], list(starts)[:k], why.value.decode()


def decode(L, z, allow, threads=4):
    n, rc = ctypes.c_size_t(), ctypes.c_int()
    p = L.bh_decode(z, len(z), threads, int(allow), ctypes.byref(n), ctypes.byref(rc))
    b = ctypes.string_at(p, n.value)
    L.bh_free(p)
    return rc.value, b


def encode(L, data, block_size, filt):
    n, rc = ctypes.c_size_t(), ctypes.c_int()
    p = L.bh_encode(data, len(data), block_size, filt, ctypes.byref(n), ctypes.byref(rc))
    b = ctypes.string_at(p, n.value)
    L.bh_free(p)
    return rc.value, b


@pytest.mark.parametrize("filt", B.FILTERS, ids=lambda f: B.NAMES[f])
def test_filters_are_liblzmas_in_both_directions(bh, filt):
    changed = 0
    for name, data, start in B.filter_cases(filt):
        for enc in (True, False):
            want = B.oracle(filt, enc, data, start)
            assert block(bh, filt, enc, data, start) == want, (name, enc)
            changed += want != data
    assert changed > 20  # the cases are not ones the filters leave alone


def test_a_start_offset_changes_the_bytes_and_the_tail_stays(bh):
    """The inputs really exercise what they are named for: positions enter the result, and a candidate in the Block's last
    4 bytes (x86), incomplete word (ARM) or halfword pair (Thumb) is left as it is."""
    for filt in B.FILTERS:
        d = B.code(filt, 5000, 1)
        assert block(bh, filt, True, d, 0) != block(bh, filt, True, d, 4096)
        cand = B._candidate(filt)
        whole = bytes(64) + cand
        assert block(bh, filt, True, whole) != whole  # converted where it is whole ...
        cutoff = whole[:-1]
        assert block(bh, filt, True, cutoff) == cutoff  # ... and not where its last byte is missing
    x = bytes(64) + B._candidate(B.X86) + bytes(3)
    assert block(bh, B.X86, True, x) != x
    x4 = bytes(64) + b"\xE8\x10\x20\x30"  # begins 4 bytes before the end
    assert block(bh, B.X86, True, x4) == x4


@pytest.mark.parametrize("filt", B.FILTERS, ids=lambda f: B.NAMES[f])
def test_the_kernels_cut_gives_the_serial_bytes(bh, filt):
    """bcj_x86_stretch_point and bcj_stretch_apply, the two routines the kernels run a lane a stretch, over every case with
    stretches of 8, 64 and 256 bytes, ascending and descending: liblzma's bytes.  Among the cases: a run of E8 bytes over
    three stretches and one over a whole 64 KiB tile, whose owner is the stretch in front."""
    for name, data, start in B.filter_cases(filt):
        for enc in (True, False):
            want = B.oracle(filt, enc, data, start)
            for stretch in (8, 64, 256):
                for order in (0, 1):
                    if len(data) > 10000 and (stretch != 256 and order):
                        continue
                    assert cut(bh, filt, enc, data, start, stretch, order) == want, (name, enc, stretch, order)


def test_x86_runs_have_one_owner(bh):
    """Inside a run of opcode bytes no position is a restart point: the stretches it covers have none, and the work of
    the run is the walk of the owner in front -- linear, whatever the data."""
    data = bytes(7) + b"\xE8" * (3 * 256 + 9) + bytes(600)
    buf = ctypes.create_string_buffer(data, len(data))
    points = (ctypes.c_uint32 * (len(data) // 256 + 1))()
    bh.bh_cut(B.X86, 1, buf, len(data), 0, 256, 0, points)
    p = list(points)[:(len(data) + 255) // 256]
    assert p[0] == 0 and p[1] == p[2] == 0xFFFFFFFF  # the run covers stretches 1 and 2 whole
    assert p[3] == (7 + 3 * 256 + 9 + 5) - 3 * 256   # five clean bytes behind the run's last byte


def test_plan_takes_the_chain_only_when_asked(bh):
    for name, z, plain in B.good_files():
        rc, bcj, starts, why = plan(bh, z, True)
        assert rc == PLAN_OK and why == "", name
        if name.startswith("liblzma_"):
            f = {v: k for k, v in B.NAMES.items()}[name.split("_")[1]]
            assert bcj == [f] and starts == [4096 if name.endswith("_start") else 0], name
            rc, _, _, why = plan(bh, z, False)
            assert rc == PLAN_UNSUPPORTED and why == "xz: unsupported filter 0x%02X" % f, name
        else:
            assert bcj == [4, 7, 0, 8, 4, 4, 7] and starts == [0, 0, 0, 0x1000, 0xFFFFFFF0, 0, 8], name
            assert plan(bh, z, False)[0] == PLAN_UNSUPPORTED


def test_plan_hands_back_every_other_chain(bh):
    for name, z, text in B.other_chain_files():
        for allow in (False, True):
            rc, _, _, why = plan(bh, z, allow)
            assert rc == PLAN_UNSUPPORTED and why == text, (name, allow, why)
    for name, z in X.unsupported_cases():  # what the plain entries promised, unchanged
        assert plan(bh, z, False)[0] == PLAN_UNSUPPORTED, name


def test_plan_refuses_properties_liblzma_refuses(bh):
    for name, z in B.refused_files():
        assert plan(bh, z, True)[0] == PLAN_FORMAT, name
        rc, _, _, why = plan(bh, z, False)
        assert rc == PLAN_UNSUPPORTED and why.startswith("xz: unsupported filter 0x0"), name


def test_host_decoder_undoes_the_filters(bh):
    for name, z, plain in B.good_files():
        for t in (1, 4):
            assert decode(bh, z, True, t) == (0, plain), (name, t)
        assert decode(bh, z, False) == (EINVAL, b""), name
    assert decode(bh, B.check_over_filtered_file(), True) == (EFORMAT, b"")
    for name, z in B.refused_files():
        assert decode(bh, z, True) == (EFORMAT, b""), name
    for name, z, plain in X.good_cases()[:6]:  # files without filters read the same with the flag
        assert decode(bh, z, True) == (0, plain), name


@pytest.mark.parametrize("filt", B.FILTERS, ids=lambda f: B.NAMES[f])
def test_host_model_with_a_filter(bh, filt):
    data = B.code(filt, 3 * 65536 + 1234, 77)
    for bs in (65536, 131072):
        rc, z = encode(bh, data, bs, filt)
        assert rc == 0
        assert lzma.decompress(z) == data
        assert decode(bh, z, True) == (0, data)
        assert decode(bh, z, False)[0] == EINVAL
        rc, bcj, starts, _ = plan(bh, z, True)
        nb = -(-len(data) // bs)
        assert bcj == [filt] * nb and starts == [0] * nb
        rc0, z0 = encode(bh, data, bs, 0)
        assert rc0 == 0 and z0 != z and lzma.decompress(z0) == data
    assert encode(bh, b"", 65536, filt) == encode(bh, b"", 65536, 0)  # no Block, no chain
    for bad in (1, 3, 5, 6, 9, 0x21):
        assert encode(bh, data[:100], 65536, bad)[0] == -1


def test_filter_helps_on_code_like_data(bh):
    """What the filter is for: calls of few targets from many places compress better behind it (the host model's sizes)."""
    data = B.x86_code(1 << 18, 5)
    assert len(encode(bh, data, 1 << 18, B.X86)[1]) < len(encode(bh, data, 1 << 18, 0)[1])


def test_same_cases_under_asan_ubsan(tmp_path):
    """Host code only, in a program of its own (tests/asan_bcj.cpp): every case from a heap buffer of exactly its size."""
    exe = hostbuild.sanitized(["tests/asan_bcj.cpp"])
    args = []
    cases = B.all_cases()
    for i, (filt, name, data, start) in enumerate(cases):
        p = tmp_path / ("c%03d" % i)
        p.write_bytes(data)
        args += [str(p), str(filt), str(start)]
    out = hostbuild.run_sanitized(exe, args)
    assert out.stdout.split() == ["ok"] * len(cases)
