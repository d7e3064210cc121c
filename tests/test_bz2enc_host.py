"""Writing data.tar.bz2 on the CPU: the host model of snappy_amd/csrc/bzip2_enc_core.h (the routines the GPU kernels run,
compiled for the host by tests/bz2enc_host_harness.cpp) over every input of tests/bz2enc_cases.py, at levels 1 and 9.
libbz2's verdict (Python's bz2) is the oracle; the project's own host decoder reads the same files through the unmodified
tests/bzip2_host_harness.cpp; the files are parsed again with bzip2_core.h's reader for what a decoder does not show (block
count, CRCs, code lengths, selector counts); the BWT stage is held against a naive sort of rotations; the size against
libbz2's on the same pieces; and a stand-alone program runs the model under ASan/UBSan.  The kernels that run the same
header are checked in tests/test_gpu_bz2enc.py."""
import bz2
import ctypes
import glob
import os
import random
import subprocess

import pytest

import bz2enc_cases as B
import xz_cases as X
from conftest import ROOT
from test_bzip2_host import bh, serial  # noqa: F401  (the decoder harness's fixture)

HARNESS = os.path.join(ROOT, "tests", "bz2enc_host_harness.cpp")
P = ctypes.POINTER
INFO = 8  # uint64 a block: be_encode's and be_parse's rows


def load_model(so_dir):
    so = os.path.join(str(so_dir), "libbz2enchost.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, HARNESS, "-pthread"])
    L = ctypes.CDLL(so)
    L.be_encode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, P(ctypes.c_size_t), P(ctypes.c_uint64), ctypes.c_size_t,
                            P(ctypes.c_size_t)]
    L.be_encode.restype = ctypes.c_void_p
    L.be_free.argtypes = [ctypes.c_void_p]
    L.be_piece.argtypes = [ctypes.c_uint32]
    L.be_piece.restype = ctypes.c_uint32
    L.be_ntables.argtypes = [ctypes.c_uint32]
    L.be_ntables.restype = ctypes.c_uint32
    L.be_rle1.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p]
    L.be_rle1.restype = ctypes.c_uint32
    L.be_bwt.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p]
    L.be_bwt.restype = ctypes.c_uint32
    L.be_code_lengths.argtypes = [P(ctypes.c_uint32), ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p]
    L.be_code_lengths.restype = None
    L.be_parse.argtypes = [ctypes.c_char_p, ctypes.c_size_t, P(ctypes.c_uint64), ctypes.c_size_t, P(ctypes.c_uint32), P(ctypes.c_uint32),
                           P(ctypes.c_uint32)]
    L.be_parse.restype = ctypes.c_int64
    return L


def encode(L, data, level, cap=64):
    """-> (the model's stream, [rle_n, orig_ptr, nmtf, ntables, nsel, crc, bits, 0] a block)"""
    n, nb = ctypes.c_size_t(), ctypes.c_size_t()
    info = (ctypes.c_uint64 * (INFO * cap))()
    p = L.be_encode(data, len(data), level, ctypes.byref(n), info, cap, ctypes.byref(nb))
    z = ctypes.string_at(p, n.value)
    L.be_free(p)
    assert nb.value <= cap
    return z, [list(info[INFO * k:INFO * k + INFO]) for k in range(nb.value)]


def parse(L, z, cap=64):
    """-> (level, stored combined CRC, folded CRC, [bit, crc, orig_ptr, ntables, nsel, longest code, n, nused] a block)"""
    rows = (ctypes.c_uint64 * (INFO * cap))()
    level, comb, fold = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    k = L.be_parse(z, len(z), rows, cap, ctypes.byref(level), ctypes.byref(comb), ctypes.byref(fold))
    assert 0 <= k <= cap, k
    return level.value, comb.value, fold.value, [list(rows[INFO * i:INFO * i + INFO]) for i in range(k)]


def rle1(L, data):
    out = ctypes.create_string_buffer(len(data) // 4 * 5 + 8)
    n = L.be_rle1(data, len(data), out)
    return out.raw[:n]


def bwt(L, data):
    out = ctypes.create_string_buffer(max(len(data), 1))
    op = L.be_bwt(data, len(data), out)
    return out.raw[:len(data)], op


def naive_bwt(b):
    """Sorted cyclic rotations, equal ones by start index: (last column, origPtr)."""
    n = len(b)
    d = b + b
    sa = sorted(range(n), key=lambda i: (d[i:i + n], i))
    return bytes(b[i - 1] for i in sa), sa.index(0)


@pytest.fixture(scope="module")
def be(tmp_path_factory):
    return load_model(tmp_path_factory.mktemp("be"))


def all_cases(be):
    def nmtf_of(d):
        return encode(be, d, 1)[1][0][2]
    return [(n, d, lv) for n, d in list(B.cases()) + B.nmtf_cases(nmtf_of) for lv in (1, 9)] + list(B.big_cases())


@pytest.fixture(scope="module")
def files(be):
    """(name, level) -> (data, the model's stream, its block infos), computed once and left alone."""
    return {(n, lv): (d,) + encode(be, d, lv) for n, d, lv in all_cases(be)}


def test_piece_sizes(be):
    assert [be.be_piece(lv) for lv in range(1, 10)] == [B.piece(lv) for lv in range(1, 10)]
    for lv in range(1, 10):
        assert B.piece(lv) % 512 == 0 and B.piece(lv) * 5 // 4 <= 100000 * lv - 19 < (B.piece(lv) + 512) * 5 // 4


def test_libbz2_reads_every_file(files):
    for (name, lv), (data, z, info) in files.items():
        assert bz2.decompress(z) == data, (name, lv)


def test_the_librarys_host_decoder_reads_every_file(files, bh):
    for (name, lv), (data, z, info) in files.items():
        rc, out = serial(bh, z)
        assert rc == 0 and out == data, (name, lv)


def test_the_files_parsed_again(files, be, bh):
    for (name, lv), (data, z, info) in files.items():
        level, comb, fold, rows = parse(be, z)
        Pn = B.piece(lv)
        assert level == lv and comb == fold, (name, lv)
        assert len(rows) == len(info) == (len(data) + Pn - 1) // Pn, (name, lv)
        for k, (row, bi) in enumerate(zip(rows, info)):
            piece = data[k * Pn:(k + 1) * Pn]
            assert row[1] == bi[5] == bh.bh_crc(piece, len(piece)), (name, lv, k)
            assert row[5] <= 17, (name, lv, k)                       # no code longer than 17 bits
            assert row[4] == bi[4] == (bi[2] + 49) // 50, (name, lv, k)  # selectors: ceil(nMTF / 50)
            assert row[3] == bi[3] == be.be_ntables(bi[2]), (name, lv, k)
            assert row[6] == bi[0] == len(rle1(be, piece)) and row[2] == bi[1], (name, lv, k)


def test_the_cases_are_what_their_names_say(files, be):
    f = {k: v for k, v in files.items()}
    Pn = B.PIECE
    for t in B.NMTF_LIMITS:
        assert f[("nmtf_%d" % t, 1)][2][0][2] == t
    assert [f[("nmtf_%d" % t, 1)][2][0][3] for t in B.NMTF_LIMITS] == [2, 3, 3, 4, 4, 5, 5, 6]
    one = f[("one_byte_3", 1)][2]
    assert len(one) == 1 and one[0][2:5] == [3, 2, 1] and parse(be, f[("one_byte_3", 1)][1])[3][0][7] == 1  # RUNA RUNA EOB; an alphabet of 3
    assert rle1(be, f[("one_byte_piece", 1)][0])[:10] == b"\0\0\0\0\xff" * 2 and f[("one_byte_piece", 1)][2][0][3:5] == [2, 1]
    assert f[("runs_of_four_piece", 1)][2][0][0] == Pn * 5 // 4 == 99840 <= 100000 - 19
    assert parse(be, f[("all_256_values", 1)][1])[3][0][7] == 256
    assert parse(be, f[("one_map_row", 1)][1])[3][0][7] == 16
    assert len(f[("six_pieces", 1)][2]) == 6
    # the runs: what RLE1 makes of them
    assert rle1(be, b"r" * 255) == b"rrrr" + bytes([251]) and rle1(be, b"r" * 259) == b"rrrr" + bytes([255])
    assert rle1(be, b"r" * 260) == b"rrrr" + bytes([255]) + b"r" and rle1(be, b"r" * 263) == b"rrrr" + bytes([255]) + b"rrrr" + bytes([0])
    assert rle1(be, b"r" * 518) == (b"rrrr" + bytes([255])) * 2
    for k in range(6):  # the run cut by the piece's end is two runs
        d = f[("run_across_%d" % k, 1)][0]
        want = b"\x07" * min(k, 4) + (bytes([k - 4]) if k >= 4 else b"")
        first = rle1(be, d[:Pn])
        assert d[Pn - k:Pn + 5 - k] == b"\x07" * 5 and d[Pn - k - 1] != 7 and first.endswith(want) and first[-len(want) - 1] != 7
    # zero runs of 2^k - 1, 2^k, 2^k + 1 in the MTF stream: ab x m has the last column b^m a^m
    for name, data in B.sorted_runs():
        last, op = bwt(be, data)
        m = len(data) // 2
        assert last == b"b" * m + b"a" * m and op == 0, name
    # a periodic block's origPtr: rotation 0 is the first of its tie group
    assert bwt(be, b"ab" * 1000) == (b"b" * 1000 + b"a" * 1000, 0)
    assert bwt(be, b"ba" * 7)[1] == 7


def test_bwt_against_a_naive_sort(be):
    r = random.Random(5)
    inputs = [b"a", b"ab", b"ba", b"aa", b"aaa", b"abab", b"abcabcabc", b"banana", b"\x00" * 64, b"ab" * 500, b"abc" * 333,
              bytes(range(256)), X.text(3000, seed=6), X.rnd(2500, seed=7), rle1(be, b"\x00" * 2590)]
    for n in (1, 2, 3, 63, 64, 65, 1023, 1024, 1025):
        inputs.append(bytes(r.randrange(3) for _ in range(n)))
    for d in inputs:
        assert bwt(be, d) == naive_bwt(d), d[:20]


def test_code_lengths_at_the_limit(be):
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    for freqs in (fib[:30], fib, [0] * 10 + fib[:28], [1] * 258, [0] * 258, [900000] + [0] * 257, [5, 0, 0]):
        arr = (ctypes.c_uint32 * len(freqs))(*freqs)
        out = ctypes.create_string_buffer(len(freqs))
        be.be_code_lengths(arr, len(freqs), 17, out)
        lens = list(out.raw)
        assert 1 <= min(lens) and max(lens) <= 17, freqs[:5]
        assert sum(2 ** (17 - l) for l in lens) == 2 ** 17, freqs[:5]  # a complete prefix code
    # the unlimited code of the Fibonacci frequencies is deeper than 17: the limit did something
    arr = (ctypes.c_uint32 * 30)(*fib[:30])
    out = ctypes.create_string_buffer(30)
    be.be_code_lengths(arr, 30, 40, out)
    assert max(out.raw) == 29


def corpus(kind, n):
    if kind == "text":
        return X.text(n, seed=77)
    if kind == "sources":
        paths = sorted(glob.glob(os.path.join(ROOT, "snappy_amd", "csrc", "*.*")) + glob.glob(os.path.join(ROOT, "tests", "*.py")))
        src = b"".join(open(p, "rb").read() for p in paths if p.endswith((".h", ".hip", ".cpp", ".inc", ".py")))
        return (src * (n // len(src) + 1))[:n] if len(src) < n else src[:n]
    so = open(os.path.join(ROOT, "snappy_amd", "libsnaphash.so"), "rb").read()  # (built_lib: it is there)
    assert len(so) >= n
    return so[:n]


@pytest.mark.parametrize("kind", ["text", "sources", "binaries"])
def test_size_against_libbz2_on_the_same_pieces(be, built_lib, kind):
    """The algorithm is libbz2's; what is left free is the length-limited code construction and the tie rules.  Measured
    (this test prints them): text 0.9998, sources 0.9999, binaries 0.9998 of libbz2's bytes."""
    data = corpus(kind, 3 * B.piece(9) // 2)
    z, info = encode(be, data, 9)
    assert bz2.decompress(z) == data
    Pn = B.piece(9)
    ref = sum(len(bz2.compress(data[o:o + Pn], 9)) for o in range(0, len(data), Pn))
    print("bz2enc size %s: model %d, libbz2 on the pieces %d, ratio %.4f" % (kind, len(z), ref, len(z) / ref))
    assert len(z) <= 1.01 * ref


def test_bz2enc_host_model_under_asan_and_ubsan(tmp_path, be):
    """Host code only, in a program of its own (tests/asan_bz2enc.cpp): the model over every input, each from a heap buffer
    of exactly its size, and 2000 random inputs of up to 200 KiB at random levels, decoded with bzip2_core.h."""
    exe = str(tmp_path / "asan_bz2enc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "asan_bz2enc.cpp"), "-pthread"])
    args = ["2000", "1"]
    cases = [c for c in all_cases(be) if c[2] == 1 or len(c[1]) <= 3000 or c in B.big_cases()]
    for i, (name, data, lv) in enumerate(cases):
        p = tmp_path / ("c%03d" % i)
        p.write_bytes(data)
        args += [str(p), str(lv)]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe] + args, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    assert out.stdout.split() == ["ok"] * len(cases) + ["random", "2000"]
