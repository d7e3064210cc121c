"""Writing data.tar.xz on the CPU: the host model of snappy_amd/csrc/xz_enc_core.h (the routines the GPU kernels run,
compiled for the host by tests/xzenc_host_harness.cpp) over every input of tests/xzenc_cases.py.  liblzma's verdict
(Python's lzma) is the oracle; the project's own host decoder reads the same files through the unmodified
tests/xz_host_harness.cpp, whose histogram shows that each shape -- matches, every rep, short reps, matched literals,
every control byte -- really occurred; the range encoder is held against xz_cases.py's Python one; xz_plan and the xz
tool judge the container; and a stand-alone program runs the model under ASan/UBSan.  The kernels that run the same
header are checked in tests/test_gpu_xzenc.py, and stage by stage -- against the arrays of stages() below -- in
tests/test_gpu_xzenc_edges.py; the tests from test_the_models_stages_make_the_models_file on show that the inputs made for
that (last Blocks of a few bytes, tiles of many hash groups, two values of one hash, distances up to a 4 MiB Block's
end, chunks on the stored / LZMA line at both places that decide it) are what their names say."""
import ctypes
import functools
import lzma
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import xz_cases as X
import xzenc_cases as E
import hostbuild
from test_xz_host import load_xh

# the decoder harness's histogram (xz_host_harness.cpp, test_xz_host.py)
H_LIT, H_MATCHED_LIT, H_MATCH, H_REP, H_SHORT_REP, H_COPY, H_CTL, H_N = 0, 1, 2, 3, 7, 10, 26, 300
# the encoder harness's statistics (xzenc_host_harness.cpp)
S_LIT, S_MATCHED_LIT, S_MATCH, S_REP, S_SHORT_REP, S_ENDS, S_CROSSES, S_CHUNKS, S_STORED, S_WATCH, S_WATCH_BYTES, S_REP0_273, S_MAX_DIST, S_MAX_SLOT, S_CODED, S_N = (
    0, 1, 2, 3, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18)
STORED = 0x80000000
SLOT = E.CHUNK + 64  # kXzEncSlot
FILL = 0xA5          # what stages() puts where the encoder writes nothing
P = ctypes.POINTER


@functools.lru_cache(maxsize=None)
def load_enc():
    """tests/xzenc_host_harness.cpp, loaded once a process with every prototype (it keeps no state between calls)."""
    L = hostbuild.shared("tests/xzenc_host_harness.cpp")
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
    vp = ctypes.c_void_p
    L.xe_stages.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64, vp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
    L.xe_stages.restype = ctypes.c_int64
    L.xe_finish.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64, vp, vp, ctypes.c_size_t, P(ctypes.c_size_t)]
    L.xe_finish.restype = ctypes.c_void_p
    L.xe_hash.argtypes = [ctypes.c_uint32]
    L.xe_hash.restype = ctypes.c_uint32
    return L


def out_cap(n):
    """XzEncBufs::out_cap: what the Blocks of a piece of n bytes take at most."""
    return n + (n + E.CHUNK - 1) // E.CHUNK * 64 + 64


def stages(L, data, block_size):
    """The model stage by stage, as the kernels leave their arrays: prev, cand (uint32 a byte, Block-relative), res (uint32
    a chunk), dst (uint64 a chunk), slots and out (bytes, FILL where nothing is written), total (bytes of out a Block)."""
    n, bs = len(data), block_size or 1 << 20
    nch, nblk = (n + E.CHUNK - 1) // E.CHUNK, (n + bs - 1) // bs
    a = {"prev": np.full(n, 0xA5A5A5A5, np.uint32), "cand": np.full(n, 0xA5A5A5A5, np.uint32), "res": np.full(nch, 0xA5A5A5A5, np.uint32),
         "dst": np.full(nch, 0xA5A5A5A5A5A5A5A5, np.uint64), "slots": np.full(nch * SLOT, FILL, np.uint8), "out": np.full(out_cap(n), FILL, np.uint8),
         "total": np.zeros(max(nblk, 1), np.uint64)}
    used = L.xe_stages(data, n, block_size, *(a[k].ctypes.data for k in ("prev", "cand", "res", "slots", "dst", "out")), out_cap(n),
                       a["total"].ctypes.data)
    assert 0 <= used <= out_cap(n)
    a["total"] = a["total"][:nblk]
    a["used"] = used
    return a


def finish(L, data, block_size, res, out, used):
    """The file from the kernels' (or the model's) out: the host's part -- headers, padding, Checks, Index -- added."""
    res, out = np.ascontiguousarray(res, np.uint32), np.ascontiguousarray(out, np.uint8)
    n = ctypes.c_size_t()
    p = L.xe_finish(data, len(data), block_size, res.ctypes.data, out.ctypes.data, used, ctypes.byref(n))
    assert p
    z = ctypes.string_at(p, n.value)
    L.xe_free(p)
    return z


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
def xe():
    return load_enc()


@pytest.fixture(scope="module")
def xh():
    return load_xh()


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
    exe = hostbuild.sanitized(["tests/asan_xzenc.cpp"])
    args = []
    for i, (name, data, bs) in enumerate(E.cases()):
        p = tmp_path / ("c%02d" % i)
        p.write_bytes(data)
        args += [str(p), str(bs)]
    out = hostbuild.run_sanitized(exe, args)
    assert out.stdout.split() == ["ok"] * len(E.cases())


# ---- the model stage by stage, and the inputs made for the kernels' own edges ---------------------------------------------


def test_the_models_stages_make_the_models_file(files, xe):
    """xe_stages (what test_gpu_xzenc_edges.py holds the kernels' arrays against) is the model of xzenc_host and no
    other: its out, with the host's part added, is the file; out differs from the file's Blocks only where the host
    writes (there it is still FILL), nothing lies behind the last Block, and an LZMA chunk's slot ends with its csize."""
    for name, (z, data, bs) in files.items():
        if name == "block_default":
            continue  # (1 MiB and 100 bytes: nothing the others do not show)
        a = stages(xe, data, bs)
        assert a["used"] == int(a["total"].sum()) == len(z) - 12 - (len(z) - plan(xe, z)[-1][3] - 8 if len(data) else 20), name
        assert finish(xe, data, bs, a["res"], a["out"], a["used"]) == z, name
        body = np.frombuffer(z, np.uint8)[12:12 + a["used"]]
        differs = a["out"][:a["used"]] != body
        assert (a["out"][:a["used"]][differs] == FILL).all() and (a["out"][a["used"]:] == FILL).all(), name
        for ci, r in enumerate(a["res"]):
            if r != STORED:
                assert (a["slots"][ci * SLOT + int(r):(ci + 1) * SLOT] == FILL).all(), (name, ci)
        if len(data):
            assert (a["prev"] != 0xA5A5A5A5).all() and (a["cand"] != 0xA5A5A5A5).all(), name  # every position has both


def test_tails_are_blocks_of_their_own_and_their_last_positions_do_not_hash(files, xe):
    for k in E.TAILS:
        z, data, bs = files["tails_%d" % k]
        assert [b[2] for b in plan(xe, z)] == [E.CHUNK, k]
        prev = stages(xe, data, bs)["prev"][E.CHUNK:]
        assert len(prev) == k and (prev[max(k - 3, 0):] == E.NONE).all(), k  # p + 4 <= blen fails
        if k > 4:  # the last position that does hash has company: a kernel that dropped it would show
            assert prev[k - 4] != E.NONE and data[E.CHUNK + int(prev[k - 4]):][:4] == data[-4:], (k, prev[k - 4])
        else:
            assert (prev == E.NONE).all()
    assert (64 - 4) // E.TILE == 0 and (65 - 4) // E.TILE == 0 and 64 // E.TILE == 1  # 65: a second tile, none of it hashes


def _tile_hashes(xe, data, t0):
    """The hashes of the positions of tile t0 that have four bytes."""
    return [xe.xe_hash(int.from_bytes(data[p:p + 4], "little")) for p in range(t0, min(t0 + E.TILE, len(data) - 3))]


def test_tile_groups_has_tiles_of_3_to_33_hashes_at_every_alignment(files, xe):
    _, data, bs = files["tile_groups"]
    _, starts = E.tile_groups()
    prev = stages(xe, data, bs)["prev"]
    assert sorted(s % E.TILE for s in starts) == sorted(set(s % E.TILE for s in starts))
    shared_seen = set()
    for p, start in zip(E.GROUP_PERIODS, starts):
        t0 = (start + E.TILE - 1) // E.TILE * E.TILE  # the first tile wholly inside the run
        assert t0 + E.TILE + 3 <= start + E.GROUP_RUN
        hs = _tile_hashes(xe, data, t0)
        shared = sum(1 for h in set(hs) if hs.count(h) > 1)
        assert len(set(hs)) == p and shared == (p if 2 * p <= E.TILE else E.TILE - p), (p, len(set(hs)), shared)
        shared_seen.add(shared)
        for q in range(max(t0, start + p), t0 + E.TILE):  # the nearest earlier position of the same hash: a period back, in or out of the tile
            assert prev[q] == q - p, (p, q)
    assert shared_seen == {3, 4, 5, 7, 16, 31, 32}  # (33 hashes in a tile: 31 of them twice)
    for t0 in range(0, len(data), E.TILE):  # and the tiles where a run begins or ends: a filler's hashes beside a period's
        hs = _tile_hashes(xe, data, t0)
        shared_seen.add(sum(1 for h in set(hs) if hs.count(h) > 1))
    assert len(shared_seen) > 7


def test_hash_twins_link_and_do_not_match(files, xe):
    _, data, bs = files["hash_twins"]
    a, b = E.twin_values()
    ia, ib = int.from_bytes(a, "little"), int.from_bytes(b, "little")
    assert a != b and a[0] != b[0] and xe.xe_hash(ia) == xe.xe_hash(ib) == E.hash32(ia) == E.hash32(ib)
    r = random.Random(3)
    for _ in range(200):
        v = r.getrandbits(32)
        assert xe.xe_hash(v) == E.hash32(v)
    st = stages(xe, data, bs)
    a1, b1, a2, b2 = E.TWIN_AT
    assert data[a1:a1 + 4] == data[a2:a2 + 4] == a and data[b1:b1 + 4] == data[b2:b2 + 4] == b
    assert a1 // E.TILE == b1 // E.TILE and b1 - a1 == 8 and a2 // E.TILE + 1 == b2 // E.TILE and b2 - a2 == 8
    for ta, tb in ((a1, b1), (a2, b2)):
        assert st["prev"][tb] == ta  # the link is there, and followed ...
        c = int(st["cand"][tb])
        assert c == 0 or tb - ((c & 0x3FFFFF) + 1) != ta, (tb, c)  # ... and is no match: none, or one from elsewhere
    assert st["prev"][a2] == b1 and int(st["cand"][a2]) == (4 << 22 | (a2 - a1 - 1))  # through the twin to the value itself


def test_far_dists_reach_the_last_distance_slots_and_the_packing_limit(files, xe):
    z, data, bs = files["far_dists"]
    assert len(data) == bs == 4 << 20 and lzma.decompress(z) == data
    _, where = E.far_dists()
    assert [d for _, d in where] == list(E.FAR_DISTS) and len(E.FAR_DISTS) == 15
    for at, d in where:
        assert data[at:at + 64] == data[at + d:at + d + 64] and 0 not in data[at:at + 64]
        s, _ = stats(xe, data, bs, watch=d)
        assert s[S_WATCH] >= 1, d
    s, res = stats(xe, data, bs, watch=E.FAR_MAX)
    assert s[S_WATCH] == 1 and s[S_WATCH_BYTES] == 273 and s[S_MAX_DIST] == E.FAR_MAX == 4194031
    assert s[S_MAX_SLOT] == 43 and len(res) == 64 and STORED not in res  # 2^21 + 2^20 <= 4 194 030 < 2^22: the format's slot 43
    st = stages(xe, data, bs)
    assert int(st["cand"][E.FAR_MAX]) == (273 << 22 | (E.FAR_MAX - 1)) and E.FAR_MAX - 1 < 1 << 22
    assert max(stats(xe, d2, b2)[0][S_MAX_SLOT] for n2, (_, d2, b2) in files.items() if n2 != "far_dists") < 40  # (block_default: 39)


def test_margin_cases_sit_on_the_stored_lzma_line(files, xe):
    """The decision 6 + csize < 3 + usize is made in two places, and S_CODED (the bytes the operations cover) tells which
    one stored a chunk: all 65 536 for the verdict after the flush, fewer for the give-up inside the loop.  margin_lzma
    is the last k written as LZMA, margin_stored the first stored one (by the verdict), margin_giveup the first one the
    loop gives up on, five bytes before its end.  (No k gives csize 65 532, the last LZMA size: the model goes from
    65 531 to stored.)"""
    assert E.MARGIN_STORED_K == E.MARGIN_LZMA_K + 1 < E.MARGIN_GIVEUP_K
    z, data, bs = files["margin_lzma"]
    s, res = stats(xe, data, bs)
    assert len(res) == 1 and res[0] != STORED and 65533 - 64 <= res[0] <= 65532, res  # 6 + csize < 3 + 65536
    assert s[S_CODED] == E.CHUNK and controls(block_payloads(xe, z)[0]) == [0xE0, 0x00]
    z, data, bs = files["margin_stored"]
    s, res = stats(xe, data, bs)
    assert res == [STORED] and s[S_CODED] == E.CHUNK and controls(block_payloads(xe, z)[0]) == [0x01, 0x00]  # the verdict
    z, data, bs = files["margin_giveup"]
    s, res = stats(xe, data, bs)
    assert res == [STORED] and E.CHUNK - 64 <= s[S_CODED] < E.CHUNK, s[S_CODED]  # the give-up, as late as it comes
    assert controls(block_payloads(xe, z)[0]) == [0x01, 0x00]
    for k in range(E.MARGIN_STORED_K, E.MARGIN_GIVEUP_K + 8):  # the line is crossed once, and so is the one between the places
        s, res = stats(xe, E.margin(k), bs)
        assert res == [STORED] and (s[S_CODED] == E.CHUNK) == (k < E.MARGIN_GIVEUP_K), (k, s[S_CODED])


def test_the_smallest_tail_chunk_written_as_lzma(files, xe):
    z, data, bs = files["tail_min"]
    _, res = stats(xe, data, bs)
    assert len(data) == E.CHUNK + E.TAIL_MIN_T and res[1] != STORED and 5 <= res[1] and 6 + res[1] < 3 + E.TAIL_MIN_T, res
    assert controls(block_payloads(xe, z)[0]) == [0xE0, 0xC0, 0x00]
    z, data, bs = files["tail_min_less"]
    _, res = stats(xe, data, bs)
    assert len(data) == E.CHUNK + E.TAIL_MIN_T - 1 and res[1] == STORED and res[0] != STORED
    assert controls(block_payloads(xe, z)[0]) == [0xE0, 0x02, 0x00]
    for t in range(1, E.TAIL_MIN_T):  # TAIL_MIN_T is the smallest
        assert stats(xe, E.tail_min(t), bs)[1][1] == STORED, t
