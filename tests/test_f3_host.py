"""Row f3 on the CPU: the host half of the data.tar.gz producer (snappy_amd/csrc/tarpack.cpp: tarCreate's
walk and member rules, ustar headers, CRC-32) and a serial model of the DEFLATE kernel's format (same
token encoder header, same chunk framing) checked against zlib, gzip and tarfile.  The kernel itself is
checked on the GPU (tests/test_gpu_f3.py)."""
import ctypes
import functools
import gzip
import io
import os
import stat
import subprocess
import tarfile
import zlib

import numpy as np
import pytest

import hostbuild
from conftest import ROOT


@functools.lru_cache(maxsize=None)
def load_f3():
    """tests/f3_host_harness.cpp, loaded once a process with every prototype.  One copy serves every module: f3_model_gzip3
    puts g_model_depth back before it returns, and f3_model_counters reports the last call only."""
    L = hostbuild.shared("tests/f3_host_harness.cpp")
    P = ctypes.POINTER
    L.f3_model_gzip.argtypes = [ctypes.c_char_p, ctypes.c_size_t, P(ctypes.c_size_t)]
    L.f3_model_gzip.restype = ctypes.c_void_p
    L.f3_model_gzip2.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, P(ctypes.c_size_t)]
    L.f3_model_gzip2.restype = ctypes.c_void_p
    L.f3_model_gzip3.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32, P(ctypes.c_size_t)]
    L.f3_model_gzip3.restype = ctypes.c_void_p
    L.f3_crc32.argtypes = [ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t]
    L.f3_crc32.restype = ctypes.c_uint32
    L.f3_crc32_combine.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]
    L.f3_crc32_combine.restype = ctypes.c_uint32
    L.f3_tar_stream.argtypes = [ctypes.c_char_p, ctypes.c_char_p, P(ctypes.c_void_p), P(ctypes.c_size_t)]
    L.f3_tar_stream_slots.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint64, P(ctypes.c_void_p), P(ctypes.c_size_t), P(ctypes.c_void_p),
                                      P(ctypes.c_size_t)]
    L.f3_tar_fill_slot_unfit.argtypes = [ctypes.c_uint64, P(ctypes.c_size_t)]
    L.f3_tar_header_of.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_void_p]
    L.f3_free.argtypes = [ctypes.c_void_p]
    L.f3_model_counters.argtypes = [ctypes.c_void_p]
    L.f3_model_counters.restype = None
    L.f3_huff_tables.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32] + [ctypes.c_void_p] * 4
    L.f3_ilog.argtypes = [ctypes.c_uint32]
    L.f3_ilog.restype = ctypes.c_uint32
    L.f3_price.argtypes = [ctypes.c_uint32] * 3
    L.f3_price.restype = ctypes.c_uint32
    return L


@pytest.fixture(scope="module")
def f3():
    return load_f3()


def sample_inputs():
    """The samples of the compressor's tests.  "segment-1" / "segment+1" keep the names they were given when a pipeline
    step took 4096 positions: 4095 and 4097 bytes are no edge of today's geometry (kDfSeg = 1920 positions, 30 tiles; a
    window of 28800 = 15 segments) -- the sizes around THAT follow them ("1920-1" ...), and tests/deflate_edge_inputs.py
    has the rest."""
    rng = np.random.default_rng(7)
    text = (b"The quick brown fox jumps over the lazy dog. " * 3000)
    words = [bytes(rng.integers(97, 123, size=int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(500)]
    prose = b" ".join(words[int(i)] for i in rng.integers(0, 500, size=40000))
    # 1 920 bytes on which the dynamic block is ONE byte smaller than the stored one: the price of the block has to leave
    # out the distance codes that exist only to complete the code (found by tools/soak_deflate.py, round 3)
    margin = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deflate_margin_1920.bin"), "rb").read()
    return {
        "stored-or-not margin": margin,
        "empty": b"", "one": b"x", "three": b"abc", "four": b"abcd", "zeros": bytes(100000), "ff": b"\xff" * 70000,
        "random": rng.integers(0, 256, size=50000, dtype=np.uint8).tobytes(), "text": text, "prose": prose,
        "random 64K": rng.integers(0, 256, size=65536, dtype=np.uint8).tobytes(), "random 200000": rng.integers(0, 256, size=200000, dtype=np.uint8).tobytes(),
        "chunk-1": prose[:65535], "chunk": prose[:65536], "chunk+1": prose[:65537], "two chunks+3": prose[:131075],
        "segment-1": prose[:4095], "segment+1": prose[:4097], "tile+1": prose[:65], "window": (prose[:30000] + b"@" + prose[:30000] + b"#") * 3,
        "long run then noise": bytes(300) + rng.integers(0, 256, size=20000, dtype=np.uint8).tobytes() + bytes(5000),
        "high bytes": bytes(rng.integers(144, 256, size=40000, dtype=np.uint8)),
        # today's segment (1920), its tile count's edges, the window (28800) and a chunk whose last segment is one byte / one tile
        "1920-1": prose[:1919], "1920": prose[:1920], "1920+1": prose[:1921], "two segments+1": prose[:3841],
        "window-1": prose[:28799], "window bytes": prose[:28800], "window+1": prose[:28801], "34 segments+1": prose[:65281],
        "chunk+tile": prose[:65536 + 64], "chunk+segment+1": prose[:65536 + 1921],
    }


def test_model_of_the_deflate_kernel_is_valid_gzip(f3):
    """Every sample decompresses (zlib's inflater and the gzip module) to exactly the input; compressible
    inputs shrink; incompressible ones cost 10 bytes per 64 KiB chunk (two stored blocks: LEN is a 16-bit field)."""
    for name, data in sample_inputs().items():
        n = ctypes.c_size_t()
        p = f3.f3_model_gzip(data, len(data), ctypes.byref(n))
        gz = ctypes.string_at(p, n.value)
        f3.f3_free(p)
        assert gz[:10] == bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 2, 0xff]), name
        assert gzip.decompress(gz) == data, name
        assert zlib.decompressobj(-15).decompress(gz[10:-8]) == data, name
        assert int.from_bytes(gz[-8:-4], "little") == zlib.crc32(data) and int.from_bytes(gz[-4:], "little") == len(data) & 0xffffffff
        n2 = ctypes.c_size_t()
        p2 = f3.f3_model_gzip2(data, len(data), 131072, ctypes.byref(n2))  # staging pieces of two chunks: no window across them
        gz2 = ctypes.string_at(p2, n2.value)
        f3.f3_free(p2)
        assert gzip.decompress(gz2) == data and len(gz2) >= len(gz) - 64, name
        if name in ("zeros", "ff", "text"):
            assert len(gz) < len(data) // 8, (name, len(gz), len(data))
        if name == "prose":  # random words out of 500: hash chains, the price parse, dynamic codes: under zlib -6 (not a parity
            # statement -- the reference's gzip-9 bytes are not reproduced -- a guard against the parse getting worse)
            assert len(gz) < len(zlib.compress(data, 6)), (name, len(gz), len(zlib.compress(data, 6)))
        if name in ("random", "random 64K", "random 200000", "high bytes"):
            assert len(gz) <= len(data) + 10 * (len(data) // 65536 + 1) + 20, (name, len(gz))


def model_with_counters(f3, data, piece, depth=0):
    """-> (the model's gzip member, its counters by name)."""
    import deflate_edge_inputs as E
    n = ctypes.c_size_t()
    p = f3.f3_model_gzip3(data, len(data), piece, depth, ctypes.byref(n))
    gz = ctypes.string_at(p, n.value)
    f3.f3_free(p)
    k = (ctypes.c_uint32 * len(E.COUNTERS))()
    f3.f3_model_counters(k)
    return gz, dict(zip(E.COUNTERS, list(k)))


def test_edge_inputs_show_the_shapes_they_are_named_for(f3):
    """tests/deflate_edge_inputs.py through the model: every input inflates to itself, and the model's counters show what the
    input was built for -- the chunk count and block kinds of each size around the segment, the window and the chunk; the
    planted repeat found at distance 28800 and not at 28801, inside a chunk and from the previous one, and not at all when
    the chunk is the first of its staging piece or four links are walked (what a depth of 1 is raised to); matches of 257 and 258 bytes, 259 cut to 258; a
    chunk with one distance symbol and one with none; and the code length code's 7-bit limiter building a second tree
    (no input is known that takes the 15-bit limiter there: the tables of test_deflate_codes_host.py do)."""
    import deflate_edge_inputs as E
    fired = 0
    for name, c in E.edge_inputs().items():
        gz, k = model_with_counters(f3, c.data, c.piece, E.effective_depth(c.depth))
        assert gzip.decompress(gz) == c.data, name
        assert k["stored"] + k["fixed"] + k["dynamic"] == k["chunks"] and k["chunks"] <= 3, (name, k)
        assert k["longest_match"] <= 258 and k["farthest_dist"] <= 28800, (name, k)
        assert k["ll_rounds"] >= 1 and (k["ll_rounds"] > 1) == (k["ll_depth"] > 15) and (k["d_rounds"] > 1) == (k["d_depth"] > 15), (name, k)
        assert (k["cl_rounds"] > 1) == (k["cl_depth"] > 7), (name, k)
        E.check_shape(name, c.want, k)
        fired += k["cl_rounds"] > 1
    assert fired >= len(E.LIMITER_SEEDS)
    # the counters themselves, on inputs whose shape needs no model to know
    _, k = model_with_counters(f3, b"", 0)
    assert k["chunks"] == 0 and k["matches"] == 0
    _, k = model_with_counters(f3, b"abcabcabcabcabcabcabcabcabcabcabcabcabcabc", 0)
    assert (k["chunks"], k["stored"], k["matches"], k["farthest_dist"], k["dist1_chunks"]) == (1, 0, 1, 3, 1), k


def test_price_arithmetic_of_the_parse(f3):
    """deflate_core.h's df_ilog / df_price, which the kernel and its model share: log2 in quarter bits, exact at the powers
    of two, never decreasing, never above the real logarithm nor 0.35 bits under it (the mantissa is linear, then cut); a price is at least one bit, at
    most its cap, and falls as the symbol gets more frequent."""
    import math
    prev = 0
    for x in list(range(1, 5000)) + [2**k + d for k in range(13, 31) for d in (-1, 0, 1)] + [2**32 - 1]:
        v = f3.f3_ilog(x)
        if x < 5000:
            assert v >= prev, x
            prev = v
        assert 4 * math.log2(x) - 1.4 < v <= 4 * math.log2(x) + 1e-9, (x, v)
    for k in range(32):
        assert f3.f3_ilog(1 << k) == 4 * k
    total = 20000
    lt = f3.f3_ilog(total + 1)
    prices = [f3.f3_price(f, lt, 56) for f in range(0, total + 1, 7)]
    assert all(4 <= p <= 56 for p in prices) and prices == sorted(prices, reverse=True)
    assert f3.f3_price(0, lt, 56) == 56 and f3.f3_price(total, lt, 56) == 4 and f3.f3_price(total // 2, lt, 56) in (4, 5)


def test_crc32_and_combine_match_zlib(f3):
    rng = np.random.default_rng(8)
    blob = rng.integers(0, 256, size=300000, dtype=np.uint8).tobytes()
    for a, b in ((0, 0), (0, 1), (1, 7), (13, 100000), (8, 8), (100001, 199999), (0, 300000)):
        assert f3.f3_crc32(0, blob[a:b], b - a) == zlib.crc32(blob[a:b])
    for cut in (0, 1, 4096, 150000, 299999, 300000):
        c1, c2 = zlib.crc32(blob[:cut]), zlib.crc32(blob[cut:])
        assert f3.f3_crc32_combine(c1, c2, len(blob) - cut) == zlib.crc32(blob)
    # the carry-less-multiplication form (tarpack.cpp crc32_clmul: 256 bytes and more) at every length class modulo 64 and
    # 16, every start alignment, and continued from a running value
    for a in range(0, 17):
        for n in list(range(240, 420)) + [1000, 4096 + a, 65536 - a, 200003]:
            assert f3.f3_crc32(0, blob[a:a + n], n) == zlib.crc32(blob[a:a + n]), (a, n)
    run = 0
    ref = 0
    for a, b in ((0, 300), (300, 1324), (1324, 1325), (1325, 70000), (70000, 300000)):
        run = f3.f3_crc32(run, blob[a:b], b - a)
        ref = zlib.crc32(blob[a:b], ref)
        assert run == ref
    assert f3.f3_crc32(0, bytes(4 << 20), 4 << 20) == zlib.crc32(bytes(4 << 20))


def _make_tree(root):
    os.makedirs(os.path.join(root, "usr", "bin"))
    os.makedirs(os.path.join(root, "meta"))
    os.makedirs(os.path.join(root, "DEBIAN"))
    os.makedirs(os.path.join(root, "DEBIAN-extra"))
    os.makedirs(os.path.join(root, "empty-dir"))
    files = {"usr/bin/foo": b"foo", "meta/package.yaml": b"name: foo", "DEBIAN/control": b"Package: foo\n",
             "DEBIAN-extra/x": b"skipped too: the rule is a string prefix", "a-b": b"", "big.bin": os.urandom(70001),
             "exactly512": bytes(512), "usr/bin/" + "n" * 90: b"long name still fits"}
    for rel, data in files.items():
        with open(os.path.join(root, rel), "wb") as f:
            f.write(data)
    os.chmod(os.path.join(root, "usr/bin/foo"), 0o755)
    os.chmod(os.path.join(root, "meta/package.yaml"), 0o640)
    os.symlink("foo", os.path.join(root, "usr", "bin", "link"))
    os.symlink("/dsafdsafsadf", os.path.join(root, "broken-link"))
    os.mkfifo(os.path.join(root, "a-fifo"))  # not regular/symlink/dir: tarCreate skips it (deb.go:290-292)
    return files


def test_tar_stream_matches_tarcreate_rules(f3, tmp_path):
    """The producer's tar stream through Python's tarfile: members, order, names, types, modes, owner, sizes,
    link targets and contents are what tarCreate would write (clickdeb/deb.go:283-341); the reference's own
    test expectations (deb_test.go: './usr/bin/foo' listed, nothing under DEBIAN) hold."""
    root = str(tmp_path / "src")
    os.makedirs(root)
    files = _make_tree(root)
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    assert f3.f3_tar_stream(root.encode(), (root + "/DEBIAN").encode(), ctypes.byref(out), ctypes.byref(n)) == 0
    stream = ctypes.string_at(out.value, n.value)
    f3.f3_free(out)
    assert len(stream) % 512 == 0 and stream[-1024:] == bytes(1024)
    tf = tarfile.open(fileobj=io.BytesIO(stream), mode="r:")
    members = tf.getmembers()
    names = [m.name for m in members]
    want = []

    def walk(d, rel):  # filepath.Walk: pre-order, byte-wise sorted per directory
        for name in sorted(os.listdir(d), key=os.fsencode):
            p, r = os.path.join(d, name), rel + "/" + name
            if p.startswith(root + "/DEBIAN"):
                continue
            st = os.lstat(p)
            if stat.S_ISREG(st.st_mode) or stat.S_ISLNK(st.st_mode) or stat.S_ISDIR(st.st_mode):
                want.append(("." + r, st))
            if stat.S_ISDIR(st.st_mode):
                walk(p, r)
    walk(root, "")
    assert names == [w[0] for w in want]
    assert "./usr/bin/foo" in names and not any("DEBIAN" in x for x in names) and "./a-fifo" not in names
    for m, (name, st) in zip(members, want):
        assert (m.uid, m.gid, m.uname, m.gname) == (0, 0, "root", "root"), name
        assert m.mtime == int(st.st_mtime), name
        assert m.mode & 0o7777 == stat.S_IMODE(st.st_mode), name
        if stat.S_ISREG(st.st_mode):
            assert m.isreg() and m.size == st.st_size and tf.extractfile(m).read() == files[name[2:]], name
        elif stat.S_ISDIR(st.st_mode):
            assert m.isdir() and m.size == 0, name
        else:
            assert m.issym() and m.linkname == os.readlink(os.path.join(root, name[2:])), name
    # raw header fields as archive/tar of the reference's era writes them
    h = stream[:512]
    assert h[257:265] == b"ustar\x0000" and h[100:108] == b"0100644\x00"[:8] or h[100:107].isdigit()
    assert h[108:116] == b"0000000\x00" and h[265:269] == b"root"
    # coreutils tar agrees
    lst = subprocess.run(["tar", "-tf", "-"], input=stream, stdout=subprocess.PIPE, check=True).stdout.decode().split("\n")
    assert [x.rstrip("/") for x in lst if x] == names


def test_tar_long_names_travel_in_pax_headers(f3, tmp_path):
    """A name or link target the ustar fields cannot hold (no slash to split at, more than 255 bytes, a target over
    100) goes out behind a PAX extended header, as Go's archive/tar falls back to (parity of its exact bytes is
    unpinned: no Go here; the check is that tarfile and coreutils tar read names, targets and contents back)."""
    root = str(tmp_path / "s")
    os.makedirs(root)
    long_file = "x" * 101                                  # no slash to split at
    deep = os.path.join("d" * 90, "e" * 90, "f" * 90)      # 272 bytes: no prefix/name split fits
    os.makedirs(os.path.join(root, deep))
    split_ok = os.path.join("p" * 80, "q" * 80)            # 161 bytes: the ustar prefix split still holds it
    os.makedirs(os.path.join(root, split_ok))
    contents = {long_file: b"long name", os.path.join(deep, "leaf"): b"deep " * 300, os.path.join(split_ok, "y"): b"split"}
    for rel, data in contents.items():
        with open(os.path.join(root, rel), "wb") as f:
            f.write(data)
    os.symlink("t" * 150, os.path.join(root, "long-link"))
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    assert f3.f3_tar_stream(root.encode(), None, ctypes.byref(out), ctypes.byref(n)) == 0
    stream = ctypes.string_at(out.value, n.value)
    f3.f3_free(out)
    tf = tarfile.open(fileobj=io.BytesIO(stream), mode="r:")
    by = {m.name: m for m in tf.getmembers()}
    for rel, data in contents.items():
        assert tf.extractfile(by["./" + rel]).read() == data, rel
    assert by["./long-link"].issym() and by["./long-link"].linkname == "t" * 150
    assert "./" + deep in by and by["./" + deep].isdir()
    assert stream.count(b" path=./") >= 3 and stream.count(b" linkpath=") == 1  # the long file, the deep directory and its leaf; the link
    assert b"PaxHeaders.0/" + long_file.encode()[:80] in stream
    raw = stream[by["./" + os.path.join(split_ok, "y")].offset:][:512]
    assert raw[156:157] == b"0" and raw[345:345 + 3] == b"./p"  # plain ustar prefix split, no PAX in front of it
    lst = subprocess.run(["tar", "-tvf", "-"], input=stream, stdout=subprocess.PIPE, check=True).stdout.decode()
    assert long_file in lst and ("t" * 150) in lst and ("f" * 90 + "/leaf") in lst


def test_tar_size_field_beyond_8_gib(f3):
    """The ustar size field holds 8 GiB - 1 in octal; a larger member gets the base-256 form (a real 8 GiB member
    would cost minutes of single-stream hashing in a test: the header alone is checked, through tarfile's parser)."""
    buf = ctypes.create_string_buffer(512)
    for size in (0, 1, (1 << 33) - 1, 1 << 33, (1 << 40) + 12345):
        assert f3.f3_tar_header_of(b"./big", ctypes.c_int64(size), buf) == 0
        ti = tarfile.TarInfo.frombuf(buf.raw, "utf-8", "surrogateescape")
        assert ti.size == size and ti.name == "./big" and ti.isreg(), size


SLOT_SIZES = (512, 1024, 1536, 4096, 65536, 0)  # 512: every record on a slot boundary; 0: the whole stream in one


def _make_slot_tree(root):
    """Every shape tar_fill_slot has a branch for: regular files around the record size and one of many records, two empty
    files next to each other, an empty file as the stream's last member, a symlink, directories, PAX members whose records
    fit one 512-byte record and PAX members whose records take two.  -> {relative path: content} of the regular files."""
    rng = np.random.default_rng(11)
    files = {"sizes/f%05d" % n: rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in (0, 1, 511, 512, 513, 1023, 1024, 1025, 70001)}
    files.update({"empties/e0": b"", "empties/e1": b"", "empties/e2-not": b"x", "zzz-last-and-empty": b""})
    files["x" * 101] = b"short PAX record: no slash to split at"
    files[os.path.join("d" * 90, "e" * 90, "f" * 90, "leaf")] = b"deep " * 300
    wide = "w" * 250
    files[os.path.join(wide, "r" * 240)] = b"r" * 513                                  # a path record of ~505 bytes: one record
    files[os.path.join(wide, "q" * 250, "p" * 240)] = b"two records of PAX data" * 50  # ~755 bytes: two
    files[os.path.join(wide, "q" * 250, "empty-behind-pax" + "o" * 200)] = b""
    for rel, data in files.items():
        os.makedirs(os.path.dirname(os.path.join(root, rel)), exist_ok=True)
        with open(os.path.join(root, rel), "wb") as f:
            f.write(data)
    os.makedirs(os.path.join(root, "empty-dir"))
    os.symlink("sizes/f00513", os.path.join(root, "link"))
    os.symlink("t" * 150, os.path.join(root, "long-link"))                             # linkpath alone: under 512
    os.symlink("t" * 400, os.path.join(root, wide, "s" * 240))                         # path + linkpath: over 512
    return files


@pytest.fixture(scope="module")
def slot_tree(f3, tmp_path_factory):
    """The tree, its stream as f3_tar_stream lays it out whole (the independent reference) and tarfile's view of that."""
    root = str(tmp_path_factory.mktemp("slots") / "src")
    os.makedirs(root)
    files = _make_slot_tree(root)
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    assert f3.f3_tar_stream(root.encode(), None, ctypes.byref(out), ctypes.byref(n)) == 0
    ref = ctypes.string_at(out.value, n.value)
    f3.f3_free(out)
    members = tarfile.open(fileobj=io.BytesIO(ref), mode="r:").getmembers()
    # the tree holds what it is meant to: the last member empty, two empty neighbours, PAX data of one record and of two
    assert members[-1].isreg() and members[-1].size == 0 and ref[-1536:] != bytes(1536) and ref[-1024:] == bytes(1024)
    assert any(a.isreg() and b.isreg() and a.size == 0 and b.size == 0 for a, b in zip(members, members[1:]))
    pax_sizes = [int(ref[o + 124:o + 135], 8) for o in range(0, len(ref) - 1024, 512) if ref[o + 156:o + 157] == b"x" and ref[o + 257:o + 262] == b"ustar"]
    assert any(s < 512 for s in pax_sizes) and any(s > 512 for s in pax_sizes), pax_sizes
    return root, files, ref, members


def _stream_in_slots(f3, root, slot_bytes):
    """-> (the stream assembled by tar_fill_slot, its segments as dicts)."""
    out, n, segs, nsegs = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_void_p(), ctypes.c_size_t()
    assert f3.f3_tar_stream_slots(root.encode(), None, slot_bytes, ctypes.byref(out), ctypes.byref(n), ctypes.byref(segs), ctypes.byref(nsegs)) == 0
    stream = ctypes.string_at(out.value, n.value)
    flat = np.frombuffer(ctypes.string_at(segs.value, nsegs.value * 56), dtype=np.uint64).reshape(-1, 7).tolist()
    f3.f3_free(out)
    f3.f3_free(segs)
    return stream, [dict(zip(("member", "s0", "slot_off", "file_off", "n", "first", "fin"), row)) for row in flat]


@pytest.mark.parametrize("slot_bytes", SLOT_SIZES)
def test_tar_fill_slot_lays_out_the_stream_slot_by_slot(f3, slot_tree, slot_bytes):
    """tarpack.cpp's tar_fill_slot, the layout the producer stages from, at slot sizes no GPU run reaches: the stream put
    together slot by slot (into a buffer of 0xA5, the segments' bytes read to their places) is f3_tar_stream's byte for byte,
    and tarfile reads every name, link target and content back from it.  The segments: none for a directory or a symlink;
    per regular member they run through the file from 0 without gap or overlap and sum to its size, lie where the member's
    content lies in the stream, the first alone has `first` and the last alone `fin`; an empty member has exactly one, of no
    bytes, with both."""
    root, files, ref, members = slot_tree
    stream, segs = _stream_in_slots(f3, root, slot_bytes)
    assert len(stream) == len(ref)
    if stream != ref:
        at = next(i for i in range(len(ref)) if stream[i] != ref[i])
        pytest.fail("slot size %d: first difference at offset %d (record %d + %d): %r, reference %r" % (slot_bytes, at, at // 512, at % 512, stream[at:at + 16], ref[at:at + 16]))
    tf = tarfile.open(fileobj=io.BytesIO(stream), mode="r:")
    got = tf.getmembers()
    assert [m.name for m in got] == [m.name for m in members] and len(got) == len(files) + sum(1 for m in members if not m.isreg())
    for m in got:
        p = os.path.join(root, m.name[2:])
        if m.isreg():
            assert tf.extractfile(m).read() == files[m.name[2:]], m.name
        elif m.issym():
            assert m.linkname == os.readlink(p), m.name
        else:
            assert m.isdir() and os.path.isdir(p), m.name
    by_member = {}
    for s in segs:
        assert members[s["member"]].isreg(), (slot_bytes, s, members[s["member"]].name)
        assert s["s0"] % (slot_bytes or len(ref)) == 0 and s["slot_off"] + s["n"] <= (slot_bytes or len(ref)), (slot_bytes, s)
        by_member.setdefault(s["member"], []).append(s)
    assert sorted(by_member) == [i for i, m in enumerate(members) if m.isreg()]
    for i, ss in by_member.items():
        m = members[i]
        at = 0
        for k, s in enumerate(ss):
            assert s["file_off"] == at and s["s0"] + s["slot_off"] == m.offset_data + at, (slot_bytes, m.name, s)
            assert (s["first"], s["fin"]) == (int(k == 0), int(k == len(ss) - 1)), (slot_bytes, m.name, ss)
            assert s["n"] > 0 or m.size == 0, (slot_bytes, m.name, ss)
            at += s["n"]
        assert at == m.size, (slot_bytes, m.name, ss)
        if m.size == 0:
            assert len(ss) == 1 and ss[0]["n"] == 0 and ss[0]["first"] == 1 and ss[0]["fin"] == 1, (slot_bytes, m.name, ss)
        if slot_bytes == 512:  # a slot a record: a segment a record of content
            assert len(ss) == max(1, (m.size + 511) // 512), (m.name, len(ss))


def test_tar_fill_slot_returns_the_header_that_does_not_fit(f3):
    """A name that neither the ustar fields nor a PAX record carry (a plan made by hand: tar_plan would add the record):
    tar_header's SNAPHASH_ENAME comes back with mi at that member, whatever the slot size."""
    from snappy_amd import _lib
    for slot_bytes in (512, 1024, 1536, 4096, 65536):
        mi = ctypes.c_size_t(99)
        assert f3.f3_tar_fill_slot_unfit(slot_bytes, ctypes.byref(mi)) == _lib.ENAME, slot_bytes
        assert mi.value == 1, slot_bytes


def test_f3_host_code_under_asan_and_ubsan(tmp_path):
    """tarpack.cpp (walk, ustar headers, CRC-32), hostsha.cpp and the serial model of the DEFLATE kernel under
    AddressSanitizer + UBSan (CPU build; GPU sanitizers are not available on the pool): a tree with every member
    kind, names at the ustar limits, and all the sample inputs."""
    src = tmp_path / "driver.cpp"
    src.write_text(r'''
#include "%s/tests/f3_host_harness.cpp"
#include "%s/snappy_amd/csrc/hostsha.cpp"
#include <stdio.h>
int main(int argc, char** argv) {
    uint8_t* out = nullptr; size_t n = 0;
    if (f3_tar_stream(argv[1], argv[2], &out, &n) != 0 || n %% 512) return 3;
    {   // the same stream from tar_fill_slot, a record a slot: every header, PAX record and padding on a slot boundary
        uint8_t* out2 = nullptr; size_t n2 = 0, nsegs = 0; uint64_t* segs = nullptr;
        if (f3_tar_stream_slots(argv[1], argv[2], 512, &out2, &n2, &segs, &nsegs) != 0 || n2 != n || memcmp(out, out2, n) != 0 || nsegs == 0) return 8;
        size_t mi = 0;
        if (f3_tar_fill_slot_unfit(512, &mi) == 0 || mi != 1) return 9;
        f3_free(out2); f3_free(segs);
    }
    size_t gz_len = 0;
    uint8_t* gz = f3_model_gzip(out, n, &gz_len);            // the tar stream through the kernel's CPU model
    if (!gz || gz_len < 18) return 4;
    snaphash::HostSha hs; uint8_t dig[64];
    snaphash::host_sha512_init(hs);
    for (size_t off = 0; off < gz_len; off += 777) snaphash::host_sha512_update(hs, gz + off, gz_len - off < 777 ? gz_len - off : 777);
    snaphash::host_sha512_final(hs, dig);
    for (size_t len : {size_t(0), size_t(1), size_t(16383), size_t(16384), size_t(16385), size_t(70000)}) {
        size_t m = 0; uint8_t* g2 = f3_model_gzip(out, len < n ? len : n, &m); f3_free(g2);
    }
    {   // the code construction alone, at its limits: ladders that are rebuilt, 320 symbols, weights beyond 16 bits
        static uint32_t freq[3 * 320], codes[3 * 320], rounds[3], depth0[3]; static uint8_t len[3 * 320];
        uint32_t a = 1, b = 1;
        for (int i = 0; i < 320; ++i) { freq[i] = i < 40 ? a : 0; freq[320 + i] = 0xffffffffu - (uint32_t)i; freq[640 + i] = i == 319; const uint32_t c = a + b; a = b; b = c; }
        if (f3_huff_tables(freq, 3, 320, 15, len, codes, rounds, depth0) != 0 || rounds[0] < 3 || rounds[1] != 1 || len[640 + 319] != 1) return 5;
        if (f3_huff_tables(freq, 1, 19, 7, len, codes, rounds, depth0) != 0 || rounds[0] < 2 || depth0[0] != 18) return 6;
        uint32_t k[16]; f3_model_counters(k);
        if (k[0] == 0) return 7;
    }
    f3_free(gz); f3_free(out);
    printf("asan f3 ok %%02x\n", dig[0]);
    return 0;
}
''' % (ROOT, ROOT))
    exe = hostbuild.sanitized([src])
    root = str(tmp_path / "src")
    os.makedirs(root)
    _make_tree(root)
    deep = os.path.join(root, *(["d" * 30] * 4))  # a 124-byte directory path: members below it need the ustar prefix split
    os.makedirs(deep)
    open(os.path.join(deep, "f" * 60), "w").write("prefix split")
    open(os.path.join(deep, "g" * 200), "w").write("PAX path record")          # beyond any ustar split
    os.symlink("t" * 300, os.path.join(deep, "pax-link"))                      # PAX linkpath record
    os.makedirs(os.path.join(root, "zz-slots"))
    _make_slot_tree(os.path.join(root, "zz-slots"))                            # sizes around the record, PAX data of two records, an empty last member
    assert "asan f3 ok" in hostbuild.run_sanitized(exe, [root, root + "/DEBIAN"]).stdout
