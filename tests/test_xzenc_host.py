"""Writing data.tar.xz on the CPU: the host model of snappy_amd/csrc/xz_enc_core.h (the routines the GPU kernels run,
compiled for the host by tests/xzenc_host_harness.cpp) over every input of tests/xzenc_cases.py.  liblzma's verdict
(Python's lzma) is the oracle; the project's own host decoder reads the same files through the unmodified
tests/xz_host_harness.cpp, whose histogram shows that each shape -- matches, every rep, short reps, matched literals,
every control byte -- really occurred; the range encoder is held against xz_cases.py's Python one; xz_plan and the xz
tool judge the container; and a stand-alone program runs the model under ASan/UBSan.  The kernels that run the same
header are checked in tests/test_gpu_xzenc.py."""
import ctypes
import lzma
import os
import random
import struct
import subprocess

import pytest

import xz_cases as X
import xzenc_cases as E
from conftest import ROOT

ENC_HARNESS = os.path.join(ROOT, "tests", "xzenc_host_harness.cpp")
DEC_HARNESS = os.path.join(ROOT, "tests", "xz_host_harness.cpp")
# the decoder harness's histogram (xz_host_harness.cpp, test_xz_host.py)
H_LIT, H_MATCHED_LIT, H_MATCH, H_REP, H_SHORT_REP, H_COPY, H_CTL, H_N = 0, 1, 2, 3, 7, 10, 26, 300
# the encoder harness's statistics (xzenc_host_harness.cpp)
S_LIT, S_MATCHED_LIT, S_MATCH, S_REP, S_SHORT_REP, S_ENDS, S_CROSSES, S_CHUNKS, S_STORED, S_WATCH, S_WATCH_BYTES, S_REP0_273, S_MAX_DIST, S_N = (
    0, 1, 2, 3, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16)
STORED = 0x80000000
P = ctypes.POINTER


def load_enc(so_dir):
    so = os.path.join(str(so_dir), "libxzenchost.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, ENC_HARNESS, "-pthread"])
    L = ctypes.CDLL(so)
    L.xe_encode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64, P(ctypes.c_size_t), P(ctypes.c_int)]
    L.xe_encode.restype = ctypes.c_void_p
    L.xe_free.argtypes = [ctypes.c_void_p]
    L.xe_stats.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32, P(ctypes.c_uint64), P(ctypes.c_uint32), ctypes.c_size_t]
    L.xe_stats.restype = ctypes.c_int64
    L.xe_rc.argtypes = [P(ctypes.c_uint32), ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_uint32]
    L.xe_rc.restype = ctypes.c_uint32
    L.xe_plan.argtypes = [ctypes.c_char_p, ctypes.c_size_t, P(ctypes.c_uint64), ctypes.c_size_t]
    L.xe_plan.restype = ctypes.c_int64
    L.xe_dict_byte.argtypes = [ctypes.c_uint64]
    L.xe_dict_byte.restype = ctypes.c_uint32
    return L


def encode(L, data, block_size):
    """(rc, file) from the host model."""
    n, rc = ctypes.c_size_t(), ctypes.c_int()
    p = L.xe_encode(data, len(data), block_size, ctypes.byref(n), ctypes.byref(rc))
    z = ctypes.string_at(p, n.value)
    L.xe_free(p)
    return rc.value, z


def stats(L, data, block_size, watch=0):
    """(statistics, every chunk's result)."""
    s = (ctypes.c_uint64 * S_N)()
    cap = len(data) // E.CHUNK + 2
    res = (ctypes.c_uint32 * cap)()
    n = L.xe_stats(data, len(data), block_size, watch, s, res, cap)
    assert 0 <= n <= cap
    return list(s), list(res[:n])


def plan(L, z):
    cap = 64
    rec = (ctypes.c_uint64 * (5 * cap))()
    n = L.xe_plan(z, len(z), rec, cap)
    assert 0 <= n <= cap, n
    return [tuple(rec[5 * i:5 * i + 5]) for i in range(n)]


def block_payloads(L, z):
    """Every Block's LZMA2 data, as xz_plan finds it."""
    return [z[o:o + ln] for o, ln, _, _, _ in plan(L, z)]


def controls(raw):
    """The control bytes of one Block's LZMA2 data, the end byte included."""
    out, at = [], 0
    while True:
        c = raw[at]
        out.append(c)
        if c == 0:
            assert at + 1 == len(raw)
            return out
        if c < 0x80:
            at += 3 + struct.unpack(">H", raw[at + 1:at + 3])[0] + 1
        else:
            assert c >= 0xC0, "every LZMA chunk resets the state and sends the properties"
            at += 6 + struct.unpack(">H", raw[at + 3:at + 5])[0] + 1


@pytest.fixture(scope="module")
def xe(tmp_path_factory):
    return load_enc(tmp_path_factory.mktemp("xe"))


@pytest.fixture(scope="module")
def xh(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("xh") / "libxzhost.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, DEC_HARNESS, "-pthread"])
    L = ctypes.CDLL(so)
    L.xh_decode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint, P(ctypes.c_size_t), P(ctypes.c_int)]
    L.xh_decode.restype = ctypes.c_void_p
    L.xh_free.argtypes = [ctypes.c_void_p]
    L.xh_hist.argtypes = [ctypes.c_char_p, ctypes.c_size_t, P(ctypes.c_uint64)]
    return L


@pytest.fixture(scope="module")
def files(xe):
    """name -> (file, input, block size): every case through the host model once."""
    out = {}
    for name, data, bs in E.cases():
        rc, z = encode(xe, data, bs)
        assert rc == 0, name
        out[name] = (z, data, bs)
    return out


def own_decode(L, z):
    n, rc = ctypes.c_size_t(), ctypes.c_int()
    p = L.xh_decode(z, len(z), 2, ctypes.byref(n), ctypes.byref(rc))
    b = ctypes.string_at(p, n.value)
    L.xh_free(p)
    return rc.value, b


def hist(L, z):
    h = (ctypes.c_uint64 * H_N)()
    assert L.xh_hist(z, len(z), h) == 0
    return list(h)


def test_liblzma_reads_every_file_back(files):
    for name, (z, data, _) in files.items():
        assert lzma.decompress(z) == data, name
        assert X.ref_decompress(z) == data, name


def test_the_projects_own_decoder_reads_every_file_back(files, xh):
    for name, (z, data, _) in files.items():
        assert own_decode(xh, z) == (0, data), name


def test_the_bytes_depend_on_input_and_block_size_alone(xe, files):
    for name in ("len_131073", "mixed_rtrt", "boundary"):
        z, data, bs = files[name]
        assert encode(xe, data, bs) == (0, z), name
    z, data, _ = files["block_default"]
    assert encode(xe, data, 1 << 20) == (0, z)  # 0 is the default, 1 MiB


def test_empty_input_is_a_stream_without_blocks(files, xe):
    z = files["len_0"][0]
    assert len(z) == 32 and plan(xe, z) == []
    assert z == X.xz_file([])


def test_block_sizes(xe):
    t = X.text(1000, 1)
    for bs in (1, 65535, 65537, 3 * 65536 + 1, (4 << 20) + 65536, 1 << 40):
        assert encode(xe, t, bs) == (-1, b""), bs
    for bs in (65536, 3 * 65536, 4 << 20):
        rc, z = encode(xe, t, bs)
        assert rc == 0 and lzma.decompress(z) == t, bs
    for bs in (65536, 3 * 65536, 1 << 20, (1 << 20) + 65536, 4 << 20):  # the smallest encodable dictionary that holds a Block
        assert xe.xe_dict_byte(bs) == X.dict_byte(bs), bs


def test_container(files, xe):
    """xz_plan accepts every file (it holds the header sizes against the Index records); the records are what the format
    decisions say: a Block per block_size bytes, the last one shorter, the dictionary the smallest that holds a Block."""
    for name, (z, data, bs) in files.items():
        bs = bs or 1 << 20
        blocks = plan(xe, z)
        want = [min(bs, len(data) - o) for o in range(0, len(data), bs)]
        assert [b[2] for b in blocks] == want, name
        assert all(b[4] == (2 | (X.dict_byte(bs) & 1)) << (X.dict_byte(bs) // 2 + 11) for b in blocks), name
        for (in_off, in_len, out_len, check_off, _), o in zip(blocks, range(0, len(data), bs)):
            assert z[check_off:check_off + 8] == struct.pack("<Q", X.crc64_fast(data[o:o + out_len])), name
        assert z[:12] == X.xz_file([])[:12] and z[-2:] == b"YZ" and z[7] == X.CHECK_CRC64


def test_block_headers_state_both_sizes(files, xe):
    for name, (z, data, bs) in files.items():
        at = 12
        for in_off, in_len, out_len, check_off, _ in plan(xe, z):
            hs = (z[at] + 1) * 4
            assert at + hs == in_off and z[at + 1] == 0xC0, name
            assert z[at + 2:].startswith(X.vli(in_len) + X.vli(out_len) + b"\x21\x01" + bytes([X.dict_byte(bs or 1 << 20)])), name
            at = check_off + 8


@pytest.mark.skipif(not os.path.exists("/usr/bin/xz"), reason="no xz tool on this machine")
def test_the_xz_tool_accepts_the_files(files, tmp_path):
    for name in ("len_0", "len_1", "len_393217", "incompressible", "mixed_rtrt", "dist_edges", "block_default"):
        p = tmp_path / (name + ".xz")
        p.write_bytes(files[name][0])
        out = subprocess.run(["/usr/bin/xz", "-t", str(p)], capture_output=True, text=True)
        assert out.returncode == 0, (name, out.stderr)


def test_incompressible_bytes_are_stored(files, xe):
    z, data, bs = files["incompressible"]
    s, res = stats(xe, data, bs)
    assert res == [STORED] * 4 and s[S_STORED] == s[S_CHUNKS] == 4
    for raw in block_payloads(xe, z):
        assert controls(raw) == [0x01, 0x02, 0x00]
        assert len(raw) == bs + 3 * 2 + 1  # usize + 3 a chunk + the end byte: the Index's unpadded size less header and Check


def test_mixed_blocks_control_bytes(files, xe):
    z, _, _ = files["mixed_rtrt"]
    (raw,) = block_payloads(xe, z)
    assert controls(raw) == [0x01, 0xC0, 0x02, 0xC0, 0x00]
    z, _, _ = files["mixed_tr"]
    (raw,) = block_payloads(xe, z)
    assert controls(raw) == [0xE0, 0x02, 0x00]
    z, _, _ = files["len_393217"]  # three Blocks and a byte: E0 C0 a Block, then one stored byte
    assert [controls(r) for r in block_payloads(xe, z)] == [[0xE0, 0xC0, 0x00]] * 3 + [[0x01, 0x00]]


def test_every_shape_occurred(files, xh):
    """From the DECODER's histogram of what the model wrote: a test that never produced a rep match has not tested one."""
    h = hist(xh, files["len_393217"][0])
    assert h[H_LIT] and h[H_MATCHED_LIT] and h[H_MATCH] and h[H_SHORT_REP]
    assert all(h[H_REP + k] for k in range(4)), h[H_REP:H_REP + 4]
    assert h[H_CTL + 0xE0] == 3 and h[H_CTL + 0xC0] == 3 and h[H_CTL + 0x01] == 1 and h[H_CTL + 0] == 4
    h = hist(xh, files["mixed_rtrt"][0])
    assert h[H_CTL + 0x01] == 1 and h[H_CTL + 0x02] == 1 and h[H_CTL + 0xC0] == 2
    for di, d in enumerate(X.COPY_DISTS):  # the copies the decoder's kernel spreads over its wave: distance 1, 63, 64, 65 at 273 bytes
        h = hist(xh, files["period_%d" % d][0])
        assert h[H_COPY + 4 * di + 3] >= 1, d
    h = hist(xh, files["all_bytes_twice"][0])
    assert h[H_LIT] == 256 and h[H_MATCH] == 1 and h[H_MATCHED_LIT] == 0  # a literal in every context, then one match
    h = hist(xh, files["sprinkled"][0])
    assert h[H_COPY + 4 * 2 + 0] >= 1 and h[H_COPY + 0] >= 1  # two bytes from 64 back and from 1 back


def test_periodic_data_rep0_and_the_cut_at_the_chunk_end(files, xe):
    for p in E.PERIODS:
        _, data, bs = files["period_%d" % p]
        s, res = stats(xe, data, bs)
        assert s[S_REP0_273] >= 1, p            # rep0 continues a match of 273 bytes
        assert s[S_ENDS] >= 1 and s[S_CROSSES] == 0, p  # chunk 0's last operation ends exactly at 65 536
        assert len(res) == 2 and all(r < 600 for r in res), (p, res)


def test_no_operation_crosses_a_chunk_end(files, xe):
    for name, (_, data, bs) in files.items():
        s, _ = stats(xe, data, bs)
        assert s[S_CROSSES] == 0, name
        assert s[S_MAX_DIST] < (bs or 1 << 20), name


def test_distance_edges(files, xe, xh):
    _, data, bs = files["dist_edges"]
    for d in E.DIST_EDGES_FAR + E.DIST_EDGES_SMALL[1:]:  # (distance 1 is rep0 after a state reset: never a new match)
        s, res = stats(xe, data, bs, watch=d)
        assert s[S_WATCH] >= 1, d
        if d >= 65535:  # the copy that reaches into an earlier chunk of its Block begins with a match of full length
            assert s[S_WATCH_BYTES] >= 273, (d, s[S_WATCH_BYTES])
    # the chunk that holds only that copy and 61 440 random bytes, which cost a little over a byte each whatever is done:
    # with the copy coded as literals the chunk would be stored (65 539); as matches the copy's 4 096 bytes all but vanish.
    # The bound asks for half of them saved.
    s, res = stats(xe, data, bs)
    first = 100 + 65535 + 65536 + 65537
    assert first // E.CHUNK == (first + 4095) // E.CHUNK == 3
    assert res[3] != STORED and res[3] < E.CHUNK - 2048, res[3]


def test_no_chain_crosses_a_block(files, xe):
    """The pattern at the end of Block 0 is no source for its copy at the start of Block 1 (liblzma refuses a distance
    past the dictionary reset: test_liblzma_reads_every_file_back): Block 1's first chunk is what it is coded alone."""
    _, data, bs = files["boundary"]
    _, res = stats(xe, data, bs)
    _, alone = stats(xe, data[bs:], bs)
    assert res[2:] == alone and len(alone) == 1
    assert alone[0] > E.BOUNDARY_PATTERN  # random bytes with no earlier copy: the pattern is paid for in literals


def _python_rc(seq):
    rc = X._RangeEncoder()
    for idx, bit in seq:
        rc.bit(idx, bit)
    return rc.finish()


def test_range_encoder_against_the_python_one(xe):
    """The same (probability index, bit) sequence through both: random bits over random indices, then >= 10 000 bits at
    one probability driven to its floor (31 / 2048) and at one driven to its ceiling (2017 / 2048), which is what makes
    runs of 0xFF cache bytes and carries into them; the bytes must be equal."""
    r = random.Random(11)
    seq = [(r.randrange(7990), r.getrandbits(1)) for _ in range(20000)]
    seq += [(5, 1)] * 400 + [(5, 1 if r.random() < 0.985 else 0) for _ in range(12000)]   # pinned near 31 / 2048
    seq += [(9, 0)] * 400 + [(9, 0 if r.random() < 0.985 else 1) for _ in range(12000)]   # pinned near 2017 / 2048
    seq += [(r.randrange(7990), r.getrandbits(1)) for _ in range(5000)]
    seq += [(5, 0)] * 3000 + [(9, 1)] * 3000  # the dear symbol over and over: the range shrinks fast, many shifts
    want = _python_rc(seq)
    idx = (ctypes.c_uint32 * len(seq))(*[i for i, _ in seq])
    bits = bytes(b for _, b in seq)
    out = ctypes.create_string_buffer(len(want) + 64)
    n = xe.xe_rc(idx, bits, len(seq), out, len(out))
    assert n == len(want) and out.raw[:n] == want
    assert b"\xff\xff" in want  # a run of pending 0xFF bytes did occur
    # a cap smaller than the output: the bytes are counted, none is written past it
    small = ctypes.create_string_buffer(b"\xaa" * 64, 64)
    assert xe.xe_rc(idx, bits, len(seq), small, 10) == n and small.raw[:10] == want[:10] and small.raw[10:] == b"\xaa" * 54


def test_xzenc_host_model_under_asan_and_ubsan(tmp_path):
    """Host code only, in a program of its own (tests/asan_xzenc.cpp): the model over every input, each from a heap
    buffer of exactly its size, and the host decoder over what it wrote."""
    exe = str(tmp_path / "asan_xzenc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "asan_xzenc.cpp"), "-pthread"])
    args = []
    for i, (name, data, bs) in enumerate(E.cases()):
        p = tmp_path / ("c%02d" % i)
        p.write_bytes(data)
        args += [str(p), str(bs)]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe] + args, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    assert out.stdout.split() == ["ok"] * len(E.cases())
