"""Row f5 on the CPU: the install side's decoder (snappy_amd/csrc/inflate_core.h, inflate_host.cpp) checked against
Python's zlib -- every block type, flush points, the gzip framing -- and its segmented form (each segment decoded on its
own with holes, then the holes filled) against the serial decode.  The GPU kernel that runs the same routine is checked
in tests/test_gpu_unpack.py and, at its edges, in tests/test_gpu_inflate_edges.py (streams: tests/inflate_edge_streams.py,
their shape on the CPU: tests/test_inflate_edges_host.py)."""
import ctypes
import functools
import gzip
import os
import random
import struct
import zlib

import numpy as np
import pytest

import hostbuild
from conftest import ROOT

HARNESS = "tests/inflate_host_harness.cpp"
EFORMAT = -9


@functools.lru_cache(maxsize=None)
def load_ih():
    """tests/inflate_host_harness.cpp, loaded once a process with every prototype (it keeps no state between calls)."""
    L = hostbuild.shared(HARNESS)
    P = ctypes.POINTER
    L.ih_gunzip.argtypes = [ctypes.c_char_p, ctypes.c_size_t, P(ctypes.c_size_t), P(ctypes.c_int)]
    L.ih_gunzip.restype = ctypes.c_void_p
    L.ih_inflate_raw.argtypes = [ctypes.c_char_p, ctypes.c_size_t, P(ctypes.c_size_t), P(ctypes.c_int), P(ctypes.c_uint64)]
    L.ih_inflate_raw.restype = ctypes.c_void_p
    L.ih_segment.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_size_t, P(ctypes.c_size_t), P(ctypes.c_int),
                             P(ctypes.c_uint64), P(ctypes.c_uint32)]
    L.ih_segment.restype = ctypes.c_void_p
    L.ih_segments.argtypes = [ctypes.c_char_p, ctypes.c_size_t, P(ctypes.c_uint64), ctypes.c_size_t, ctypes.c_uint, P(ctypes.c_size_t),
                              P(ctypes.c_int)]
    L.ih_segments.restype = ctypes.c_void_p
    L.ih_candidates.argtypes = [ctypes.c_char_p, ctypes.c_size_t, P(ctypes.c_uint64), ctypes.c_size_t]
    L.ih_candidates.restype = ctypes.c_size_t
    L.ih_free.argtypes = [ctypes.c_void_p]
    return L


@pytest.fixture(scope="module")
def ih():
    return load_ih()


def _take(L, p, n):
    b = ctypes.string_at(p, n)
    L.ih_free(p)
    return b


def gunzip(L, gz):
    n, rc = ctypes.c_size_t(), ctypes.c_int()
    out = _take(L, L.ih_gunzip(gz, len(gz), ctypes.byref(n), ctypes.byref(rc)), n.value)
    return rc.value, out


def inflate_raw(L, raw):
    n, st, end = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_uint64()
    out = _take(L, L.ih_inflate_raw(raw, len(raw), ctypes.byref(n), ctypes.byref(st), ctypes.byref(end)), n.value)
    return st.value, end.value, out


def segments(L, raw, starts, threads=3):
    arr = (ctypes.c_uint64 * len(starts))(*starts)
    n, rc = ctypes.c_size_t(), ctypes.c_int()
    out = _take(L, L.ih_segments(raw, len(raw), arr, len(starts), threads, ctypes.byref(n), ctypes.byref(rc)), n.value)
    return rc.value, out


def corpora():
    rng = np.random.default_rng(11)
    words = [bytes(rng.integers(97, 123, size=int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(700)]
    prose = b" ".join(words[int(i)] for i in rng.integers(0, 700, size=60000))
    src = open(os.path.join(ROOT, "snappy_amd", "csrc", "snaphash_api.cpp"), "rb").read()[:200000]
    return {
        "empty": b"", "one": b"x", "prose": prose, "sources": src, "zeros": bytes(200000),
        "random": rng.integers(0, 256, size=150000, dtype=np.uint8).tobytes(),
        "mixed": prose[:50000] + rng.integers(0, 256, size=30000, dtype=np.uint8).tobytes() + bytes(70000) + src[:40000],
    }


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=(), mode=zlib.Z_SYNC_FLUSH):
    """Raw DEFLATE of data with a flush (mode) after each offset in flushes; returns the stream and the byte offsets
    at which each flush left it (segment starts)."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, starts, at = [], [], 0
    for f in sorted(set(flushes)):
        if not 0 < f < len(data):
            continue
        out.append(c.compress(data[at:f]))
        out.append(c.flush(mode))
        starts.append(sum(len(x) for x in out))
        at = f
    out.append(c.compress(data[at:]))
    out.append(c.flush())
    return b"".join(out), starts


@pytest.mark.parametrize("level", [0, 1, 6, 9])
def test_levels_match_zlib(ih, level):
    for name, data in corpora().items():
        for strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED):
            raw, _ = raw_deflate(data, level, strategy)
            st, end, out = inflate_raw(ih, raw)
            assert st == 0 and out == data, (name, level, strategy)
            assert (end + 7) // 8 == len(raw), name


def test_gzip_framing_and_crc(ih):
    for name, data in corpora().items():
        rc, out = gunzip(ih, gzip.compress(data, 9))
        assert rc == 0 and out == data, name


def test_flush_points_at_random(ih):
    r = random.Random(5)
    for name, data in corpora().items():
        if len(data) < 10:
            continue
        for mode in (zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH):
            flushes = [r.randrange(1, len(data)) for _ in range(r.randrange(1, 40))]
            raw, _ = raw_deflate(data, r.choice([1, 6, 9]), flushes=flushes, mode=mode)
            st, _, out = inflate_raw(ih, raw)
            assert st == 0 and out == data, (name, mode)


class BitWriter:
    def __init__(self):
        self.bits, self.n, self.out = 0, 0, bytearray()

    def put(self, v, k):
        self.bits |= v << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.bits & 255)
            self.bits >>= 8
            self.n -= 8

    def huff(self, code, k):  # Huffman codes go most significant bit first
        self.put(int(format(code, "0%db" % k)[::-1], 2), k)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)


def fixed_lit(w, sym):
    if sym < 144:
        w.huff(0x30 + sym, 8)
    elif sym < 256:
        w.huff(0x190 + sym - 144, 9)
    elif sym < 280:
        w.huff(sym - 256, 7)
    else:
        w.huff(0xc0 + sym - 280, 8)


def test_long_matches_and_farthest_distance_across_a_flush(ih):
    rng = np.random.default_rng(3)
    block = rng.integers(0, 256, size=30000, dtype=np.uint8).tobytes()
    # zlib: the second copy of `block` lies 30 000 bytes back and the flushes cut the copy -- the matches after them
    # reach across the segment start (holes), 258-byte matches throughout
    data = block + block + block[:5000] + bytes(4000)
    raw, starts = raw_deflate(data, 9, flushes=[30000 + 100, 30000 + 20000])
    st, _, out = inflate_raw(ih, raw)
    assert st == 0 and out == data
    rc, out = segments(ih, raw, [0] + starts)
    assert rc == 0 and out == data
    n, stt, end, he = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_uint64(), ctypes.c_uint32()
    p = ih.ih_segment(raw, len(raw), starts[0] * 8, 1 << 20, ctypes.byref(n), ctypes.byref(stt), ctypes.byref(end), ctypes.byref(he))
    syms = np.frombuffer(_take(ih, p, 2 * n.value), dtype=np.uint16)
    assert stt.value == 1 and end.value == starts[1] * 8
    holes = syms[syms >= 256] - 256
    assert holes.size > 0 and holes.max() <= 30100 and np.all(syms[he.value:] < 256)

    # zlib never reaches 32 768 back (its MAX_DIST is 32 506): a hand-made stream does -- 32 768 stored bytes, a
    # Z_SYNC_FLUSH marker, then a fixed block of 258-byte matches at distance 32 768 (length code 285, distance code 29
    # with 13 extra bits of 8191)
    w = BitWriter()
    w.put(0, 3)
    w.align()
    w.out += struct.pack("<HH", 32768, 0x7fff) + bytes(block[:32768] if len(block) >= 32768 else (block * 2)[:32768])
    w.put(0, 3)
    w.align()
    w.out += b"\x00\x00\xff\xff"
    seg_start = len(w.out)
    w.put(1, 1)
    w.put(1, 2)
    for _ in range(200):
        fixed_lit(w, 285)
        w.huff(29, 5)
        w.put(8191, 13)
    fixed_lit(w, 256)
    w.align()
    far = bytes(w.out)
    first = (block * 2)[:32768]
    want = bytearray(first)
    for _ in range(200 * 258):
        want.append(want[-32768])
    st, _, out = inflate_raw(ih, far)
    assert st == 0 and out == bytes(want)
    rc, out = segments(ih, far, [0, seg_start])
    assert rc == 0 and out == bytes(want)
    p = ih.ih_segment(far, len(far), seg_start * 8, 1 << 20, ctypes.byref(n), ctypes.byref(stt), ctypes.byref(end), ctypes.byref(he))
    syms = np.frombuffer(_take(ih, p, 2 * n.value), dtype=np.uint16)
    assert stt.value == 0 and n.value == 200 * 258
    assert syms[0] == 256 + 32768 and np.all(syms >= 256)  # every byte of the segment is a hole: a copy of a copy
    assert he.value == n.value


def test_stored_chunk_containing_the_flush_marker(ih):
    rng = np.random.default_rng(9)
    noise = bytearray(rng.integers(0, 256, size=100000, dtype=np.uint8).tobytes())
    for at in (10, 5000, 40000, 70000, 99990):
        noise[at:at + 4] = b"\x00\x00\xff\xff"
    data = bytes(noise)
    raw, starts = raw_deflate(data, 0, flushes=[30000, 60000])
    n = ctypes.c_size_t
    cand = (ctypes.c_uint64 * 64)()
    k = ih.ih_candidates(raw, len(raw), cand, 64)
    assert k > len(starts)  # false candidates inside the stored data
    assert set(starts) <= set(cand[:k])
    st, _, out = inflate_raw(ih, raw)
    assert st == 0 and out == data
    rc, out = segments(ih, raw, [0] + starts)
    assert rc == 0 and out == data
    # cut at a false candidate: the chain does not link
    false = [c for c in cand[:k] if c not in starts][0]
    rc, _ = segments(ih, raw, sorted([0, false] + starts))
    assert rc == EFORMAT


def test_concatenated_members_and_every_header_field(ih):
    a, b = b"first member " * 1000, bytes(range(256)) * 300
    name, comment, extra = b"data.tar", b"a comment", b"AB\x04\x00wxyz"

    def member(data, flg):
        hdr = bytearray(b"\x1f\x8b\x08" + bytes([flg]) + b"\x00\x00\x00\x00\x00\x03")
        if flg & 4:
            hdr += struct.pack("<H", len(extra)) + extra
        if flg & 8:
            hdr += name + b"\x00"
        if flg & 16:
            hdr += comment + b"\x00"
        if flg & 2:
            hdr += struct.pack("<H", zlib.crc32(bytes(hdr)) & 0xffff)
        c = zlib.compressobj(9, zlib.DEFLATED, -15)
        return bytes(hdr) + c.compress(data) + c.flush() + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)

    for flg in (0, 2, 4, 8, 16, 2 | 4 | 8 | 16):
        gz = member(a, flg) + member(b, flg) + member(b"", flg)
        rc, out = gunzip(ih, gz)
        assert rc == 0 and out == a + b, flg
        assert gzip.decompress(gz) == out
    bad_hcrc = bytearray(member(a, 2 | 8))
    bad_hcrc[10 + len(name) + 1] ^= 1
    assert gunzip(ih, bytes(bad_hcrc))[0] == EFORMAT
    assert gunzip(ih, member(a, 0) + b"\x00")[0] == EFORMAT  # trailing bytes that are no member


def test_f3_model_archives(ih):
    """The compressor's CPU model (tests/deflate_model.h through the f3 harness): its archives decode, and their flush
    points cut them into segments that decode on their own."""
    from test_f3_host import load_f3
    f3 = load_f3()
    c = corpora()
    for name in ("prose", "sources", "zeros", "random", "mixed"):
        data = c[name] * 2
        n = ctypes.c_size_t()
        p = f3.f3_model_gzip(data, len(data), ctypes.byref(n))
        gz = ctypes.string_at(p, n.value)
        f3.f3_free(p)
        rc, out = gunzip(ih, gz)
        assert rc == 0 and out == data, name
        raw = gz[10:-8]
        k = ih.ih_candidates(raw, len(raw), None, 0)
        cand = (ctypes.c_uint64 * max(k, 1))()
        ih.ih_candidates(raw, len(raw), cand, k)
        chunks = (len(data) + 65535) // 65536
        assert k >= chunks - 1, name  # one flush point after every 64 KiB chunk
        # link the chain as the engine does: each segment starts where the one before it ended, at a candidate
        chain, at, cset = [0], 0, set(cand[:k])
        n2, st, end, he = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_uint64(), ctypes.c_uint32()
        while True:
            ih.ih_free(ih.ih_segment(raw, len(raw), at * 8, 1 << 20, ctypes.byref(n2), ctypes.byref(st), ctypes.byref(end), ctypes.byref(he)))
            if st.value == 0:
                break
            assert st.value == 1 and end.value % 8 == 0 and end.value // 8 in cset, name
            at = end.value // 8
            chain.append(at)
        assert len(chain) >= chunks, name
        rc, out = segments(ih, raw, chain)
        assert rc == 0 and out == data, name


def test_random_segmentations_match_the_serial_decode(ih):
    r = random.Random(17)
    c = corpora()
    for trial in range(24):
        data = c[r.choice(["prose", "sources", "mixed", "zeros", "random"])]
        flushes = [r.randrange(1, len(data)) for _ in range(r.randrange(2, 30))]
        raw, starts = raw_deflate(data, r.choice([1, 6, 9]), flushes=flushes, mode=r.choice([zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH]))
        starts = sorted(set(starts))
        subset = [0] + sorted(r.sample(starts, r.randrange(0, len(starts) + 1)))
        rc, out = segments(ih, raw, subset, threads=r.choice([1, 4]))
        assert rc == 0 and out == data, trial


def test_truncated_and_mutated_streams_are_refused(ih):
    data = corpora()["prose"]
    gz = gzip.compress(data, 6)
    r = random.Random(1)
    for cut in [0, 1, 9, 10, 11, len(gz) // 2, len(gz) - 9, len(gz) - 1]:
        assert gunzip(ih, gz[:cut])[0] == EFORMAT, cut
    bad_crc = bytearray(gz)
    bad_crc[-8] ^= 1
    assert gunzip(ih, bytes(bad_crc))[0] == EFORMAT
    bad_len = bytearray(gz)
    bad_len[-1] ^= 1
    assert gunzip(ih, bytes(bad_len))[0] == EFORMAT
    for _ in range(300):
        m = bytearray(gz)
        for _ in range(r.randrange(1, 5)):
            m[r.randrange(10, len(m))] = r.randrange(256)
        rc, out = gunzip(ih, bytes(m))
        assert rc in (0, EFORMAT)
        if rc == 0:
            assert zlib.decompress(bytes(m), 31) == out


def test_inflate_host_code_under_asan_and_ubsan(tmp_path):
    exe = hostbuild.sanitized([HARNESS], defines=["IH_MAIN"])
    c = corpora()
    data = c["prose"][:20000] + c["random"][:3000] + bytes(3000)
    raw, _ = raw_deflate(data, 6, flushes=[4000, 9000, 15000, 21000])
    gzf = tmp_path / "in.gz"
    gzf.write_bytes(b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + raw + struct.pack("<II", zlib.crc32(data), len(data)))
    hostbuild.run_sanitized(exe, [gzf, 20000, 7], timeout=900)
