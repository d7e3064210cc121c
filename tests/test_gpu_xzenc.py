"""Writing data.tar.xz on the GPU: snaphash_xz_buffer (lzma_chains_kernel, lzma2_chunks_kernel, lzma2_concat_kernel and
the CRC-64 kernels) and snaphash_tar_create_xz, in both configurations (conftest.py snaphash_mode), over the inputs of
tests/xzenc_cases.py.  liblzma's verdict (Python's lzma) carries the tests; the bytes are also held against the host
model of the same header (tests/xzenc_host_harness.cpp) -- a self-comparison that shows no lane, workgroup, slot or launch
leaks into the output -- and the library's own install side reads every file back, a Block a workgroup."""
import bz2
import ctypes
import hashlib
import io
import lzma
import os
import subprocess
import tarfile
import zlib

import numpy as np
import pytest

import trees
import xz_cases as X
import xzenc_cases as E
from conftest import ROOT
from snappy_amd import Context, _lib, clickdeb
from test_f3_host import f3  # noqa: F401  (f3_tar_stream: the tar stream laid out whole)
from test_xzenc_host import encode, load_enc, plan

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "snappy_amd", "bin", "snaphash")


@pytest.fixture(scope="module")
def xe():
    return load_enc()


@pytest.fixture(scope="module")
def model(xe):
    """name -> the host model's file, computed once and left alone."""
    out = {}
    for name, data, bs in E.cases():
        rc, z = encode(xe, data, bs)
        assert rc == 0, name
        out[name] = z
    return out


def test_xz_buffer_on_every_input(snaphash_mode, model):
    with Context(device=0) as c:
        for name, data, bs in E.cases():
            z = c.xz_buffer(data, bs)
            assert lzma.decompress(z) == data, name
            assert z == model[name], name
            st = c.targz_stats()
            chunks = sum((min(bs or 1 << 20, len(data) - o) + E.CHUNK - 1) // E.CHUNK for o in range(0, len(data), bs or 1 << 20))
            assert st["tar_bytes"] == len(data) and st["gz_bytes"] == len(z) and st["chunks"] == chunks, (name, st)
            if name == "incompressible":
                assert st["stored_chunks"] == st["chunks"] == 4
            if name == "mixed_rtrt":
                assert st["stored_chunks"] == 2
            if name.startswith("period_"):
                assert st["stored_chunks"] == 0


def test_refused_block_sizes_and_a_ctx_that_survives(snaphash_mode, model):
    name, data, bs = E.by_name("len_131073")
    with Context(device=0) as c:
        for bad in (1, 65535, 65537, (4 << 20) + 65536, 1 << 40):
            with pytest.raises(_lib.SnaphashError) as e:
                c.xz_buffer(data, bad)
            assert e.value.code == _lib.EINVAL, bad
        assert c.xz_buffer(data, bs) == model[name]
        assert c.xz_buffer(b"") == model["len_0"] and len(model["len_0"]) == 32


def test_the_bytes_do_not_depend_on_slots_or_launches(snaphash_mode, xe):
    """384 KiB in one call, and again by engines whose staging cuts it into three slots of one Block, and into six of a
    64 KiB Block each; a ctx that has compressed something else before gives the same bytes too."""
    data = X.text(384 * 1024, 70)
    with Context(device=0) as c:
        whole = c.xz_buffer(data, 128 * 1024)
        assert c.xz_buffer(X.rnd(100000, 71), 65536) != whole
        assert c.xz_buffer(data, 128 * 1024) == whole
        whole64 = c.xz_buffer(data, 65536)
    assert lzma.decompress(whole) == data and (0, whole) == encode(xe, data, 128 * 1024)
    with Context(device=0, staging_bytes=128 * 1024) as c:
        assert c.xz_buffer(data, 128 * 1024) == whole
        assert c.targz_stats()["chunks"] == 6
    with Context(device=0, staging_bytes=65536) as c:
        assert c.xz_buffer(data, 65536) == whole64
        with pytest.raises(_lib.SnaphashError) as e:  # a Block must fit the engine's staging
            c.xz_buffer(data, 128 * 1024)
        assert e.value.code == _lib.EINVAL


def _encoder_calls(data):
    """The build side's buffer calls, one format after the other and each format twice with other parameters:
    (what to call on a Context, Python's decoder, what the stream's header must say)."""
    return [
        (lambda c: c.xz_buffer(data, 65536, 1), lzma.decompress, lambda z: z[:6] == b"\xfd7zXZ\x00" and z[6:8] == b"\x00\x01"),
        (lambda c: c.bzip2_buffer(data, 1), bz2.decompress, lambda z: z[:4] == b"BZh1"),
        (lambda c: c.gzip_buffer(data), lambda z: zlib.decompress(z, 31), lambda z: z[:3] == b"\x1f\x8b\x08"),
        (lambda c: c.xz_buffer(data), lzma.decompress, lambda z: z[:6] == b"\xfd7zXZ\x00" and z[6:8] == b"\x00\x04"),
        (lambda c: c.bzip2_buffer(data, 9), bz2.decompress, lambda z: z[:4] == b"BZh9"),
        (lambda c: c.gzip_buffer(data), lambda z: zlib.decompress(z, 31), lambda z: z[:3] == b"\x1f\x8b\x08"),
    ]


@pytest.mark.kernels_only("the encoders hold the same state in both configurations: no call here hashes a member")
def test_encoder_state_is_the_calls_own(snaphash_mode, tmp_path, f3):
    """An encoder's parameters and running state belong to one call: six buffer calls in one Context -- .xz with a 64 KiB
    Block and CRC-32, .bz2 at level 1, gzip, .xz with the default Block and Check, .bz2 at level 9, gzip again -- each decode
    (lzma, bz2, zlib) to the input, say in their header what was asked (the Check id, the level), and are byte for byte what
    the same call gives as the first of a fresh Context of the same staging size; then a .tar.bz2 and a .tar.xz of a small
    tree in that Context carry f3_tar_stream's stream at level 9 and with CRC-64.

    The staging size is 1 MiB: the smallest that admits every call of the list (a Block of the default 1 MiB and a level 9
    block's 719 872 bytes of input must fit the staging; an engine of 128 KiB refuses both, as the test above and
    test_gpu_bz2enc.py pin for smaller engines).  The 128 KiB engine follows with the calls it admits, which then take two
    and three slots each -- the Index records, the carried bits and the CRC go from slot to slot -- and with its refusals,
    after which it still gives the same bytes."""
    rng = np.random.default_rng(90)
    n = 3 * 65536 + 1
    data = X.text(n // 2, 91) + rng.integers(0, 256, size=n - n // 2, dtype=np.uint8).tobytes()
    calls = _encoder_calls(data)

    def fresh(staging, k):
        with Context(device=0, staging_bytes=staging) as c:
            return calls[k][0](c)

    root = str(tmp_path / "src")
    os.makedirs(os.path.join(root, "d"))
    for rel, content in (("a", b"a" * 1000), ("d/b", data[:70001]), ("d/empty", b"")):
        with open(os.path.join(root, rel), "wb") as fh:
            fh.write(content)
    p, ln = ctypes.c_void_p(), ctypes.c_size_t()
    assert f3.f3_tar_stream(root.encode(), None, ctypes.byref(p), ctypes.byref(ln)) == 0
    tar = ctypes.string_at(p.value, ln.value)
    f3.f3_free(p)

    with Context(device=0, staging_bytes=1 << 20) as c:
        outs = []
        for k, (call, decode, header_ok) in enumerate(calls):
            z = call(c)
            assert decode(z) == data, k
            assert header_ok(z), (k, z[:8])
            assert z == fresh(1 << 20, k), k
            outs.append(z)
        assert outs[2] == outs[5] and outs[0] != outs[3] and outs[1] != outs[4]
        out_bz, out_xz = str(tmp_path / "t.tar.bz2"), str(tmp_path / "t.tar.xz")
        c.tar_create_bz2(out_bz, root)
        raw = open(out_bz, "rb").read()
        assert bz2.decompress(raw) == tar and raw[:4] == b"BZh9"
        c.tar_create_xz(out_xz, root)
        raw = open(out_xz, "rb").read()
        assert lzma.decompress(raw) == tar and raw[6:8] == b"\x00\x04"

    with Context(device=0, staging_bytes=128 * 1024) as c:
        for k in (0, 1, 2, 3, 4, 5, 0, 1):
            call, decode, header_ok = calls[k]
            if k in (3, 4):  # a Block, a block's input, larger than the engine's staging: refused, and the engine goes on
                with pytest.raises(_lib.SnaphashError) as e:
                    call(c)
                assert e.value.code == _lib.EINVAL and "larger than the engine's staging size" in str(e.value), k
                continue
            z = call(c)
            assert decode(z) == data and header_ok(z), k
            assert c.targz_stats()["tar_bytes"] == n, k
            assert z == fresh(128 * 1024, k), k
            if k != 2 and k != 5:  # (.xz and .bz2 depend on no slot size; a gzip chunk's window ends at its slot's start)
                assert z == outs[k], k


def test_round_trip_through_the_librarys_own_install_side(snaphash_mode, model):
    with Context(device=0) as c:
        for name, data, bs in E.cases():
            assert c.unxz_buffer(model[name]) == data, name
            st = c.unpack_stats()
            bsz = bs or 1 << 20
            assert st["segments"] == (len(data) + bsz - 1) // bsz, (name, st)
            if snaphash_mode == "gpu_only":  # every Block this side writes is one the kernel takes
                assert st["gpu_segments"] == st["segments"] and st["host_bytes"] == 0, (name, st)


def _make_tree(root):
    """The small tree of test_gpu_f3.py / test_f3_host.py."""
    for d in ("usr/bin", "meta", "DEBIAN", "DEBIAN-extra", "empty-dir"):
        os.makedirs(os.path.join(root, d))
    files = {"usr/bin/foo": b"foo", "meta/package.yaml": b"name: foo", "DEBIAN/control": b"Package: foo\n",
             "DEBIAN-extra/x": b"skipped too: the rule is a string prefix", "a-b": b"", "big.bin": X.rnd(70001, 80),
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


def test_tar_create_xz_matches_tarfiles_view_of_the_tree(snaphash_mode, tmp_path, xe):
    root = str(tmp_path / "src")
    os.makedirs(root)
    files = _make_tree(root)
    out = str(tmp_path / "data.tar.xz")
    with Context(device=0) as c:
        _, digest = c.tar_create_xz(out, root, root + "/DEBIAN")
        st = c.targz_stats()
        raw = open(out, "rb").read()
        assert hashlib.sha512(raw).digest() == digest and st["gz_bytes"] == len(raw) and st["members"] >= 10
        tar = lzma.decompress(raw)
        assert st["tar_bytes"] == len(tar) and len(tar) % 512 == 0 and st["chunks"] == (len(tar) + E.CHUNK - 1) // E.CHUNK
        assert (0, raw) == encode(xe, tar, 0)  # Blocks of the default size, the host model's bytes
        assert [b[2] for b in plan(xe, raw)] == [min(1 << 20, len(tar) - o) for o in range(0, len(tar), 1 << 20)]
        tf = tarfile.open(fileobj=io.BytesIO(raw), mode="r:xz")
        names = tf.getnames()
        assert "./usr/bin/foo" in names and not any("DEBIAN" in n for n in names) and "./a-fifo" not in names
        for m in tf.getmembers():
            assert (m.uid, m.gid, m.uname, m.gname) == (0, 0, "root", "root")
            if m.isreg():
                assert tf.extractfile(m).read() == files[m.name[2:]], m.name
        assert tf.getmember("./usr/bin/link").linkname == "foo" and tf.getmember("./usr/bin/foo").mode & 0o777 == 0o755
        # over a longer file, a shorter file and a fresh path: the same bytes
        for old in (X.rnd(len(raw) + 70001, 81), b"short", None):
            if old is None:
                os.unlink(out)
            else:
                with open(out, "wb") as f:
                    f.write(old)
            assert c.tar_create_xz(out, root, root + "/DEBIAN")[1] == digest and open(out, "rb").read() == raw
        # the gzip producer's bytes carry the same tar stream
        gz = str(tmp_path / "data.tar.gz")
        c.tar_create(gz, root, root + "/DEBIAN")
        import gzip
        assert gzip.decompress(open(gz, "rb").read()) == tar
        for bad in (gz, str(tmp_path / "data.tar"), str(tmp_path / "data.tar.bz2")):
            before = os.path.exists(bad) and open(bad, "rb").read()
            with pytest.raises(_lib.SnaphashError) as e:
                c.tar_create_xz(bad, root, root + "/DEBIAN")
            assert e.value.code == _lib.EINVAL and "unknown compression extension" in str(e.value)
            assert (os.path.exists(bad) and open(bad, "rb").read()) == before
        # clickdeb.tarCreate dispatches on the suffix as deb.go:269-276 does
        assert clickdeb.tarCreate(str(tmp_path / "cd.tar.xz"), root, ctx=c) == hashlib.sha512(open(str(tmp_path / "cd.tar.xz"), "rb").read()).digest()
        assert "./DEBIAN/control" in tarfile.open(str(tmp_path / "cd.tar.xz"), "r:xz").getnames()  # (tarCreate's fn = None keeps all)
        clickdeb.tarCreate(str(tmp_path / "cd.tar.gz"), root, ctx=c)
        with pytest.raises(_lib.SnaphashError) as e:
            clickdeb.tarCreate(str(tmp_path / "cd.tar.zst"), root, ctx=c)
        assert "unknown compression extension" in str(e.value)


def test_fused_hashes_yaml_and_the_way_back(snaphash_mode, oracle, tmp_path):
    """tar + .xz + archive digest + per-file SHA-512 + hashes.yaml from one read, over slots of two Blocks (2 MiB
    staging); then the archive unpacked again by snaphash_tar_unpack_xz with the yaml just produced."""
    sizes = [0, 1, 511, 512, 513, 4096, 65536, 65537, 100000, 300000, 700001, (1 << 20) + 77]
    build, _ = trees.make_synthetic_tree(str(tmp_path), sizes)
    with open(os.path.join(build, "d0000", "text.txt"), "wb") as f:
        f.write(X.text(400000, 82))
    os.makedirs(os.path.join(build, "DEBIAN"))
    with open(os.path.join(build, "DEBIAN", "control"), "w") as f:
        f.write("Package: x\n")
    out = str(tmp_path / "data.tar.xz")
    with Context(device=0, staging_bytes=2 << 20) as c:
        yaml, digest = c.tar_create_xz(out, build, build + "/DEBIAN", with_hashes=True)
        zs = c.targz_stats()
        assert 0 < zs["stored_chunks"] < zs["chunks"] and zs["gz_bytes"] == os.path.getsize(out)
        assert c.tree(build, out) == yaml
        mis, dig2 = c.tar_unpack_xz(out, str(tmp_path / "unpacked"), yaml)
        assert mis is None and dig2 == digest
        us = c.unpack_stats()
        assert us["segments"] == (zs["tar_bytes"] + (1 << 20) - 1) >> 20
        if snaphash_mode == "gpu_only":
            assert us["gpu_segments"] == us["segments"]
    assert oracle.hashes_yaml(build, out) == yaml
    assert hashlib.sha512(open(out, "rb").read()).digest() == digest
    tf = tarfile.open(out, "r:xz")
    for m in tf.getmembers():
        if m.isreg():
            assert tf.extractfile(m).read() == open(os.path.join(build, m.name[2:]), "rb").read(), m.name
            assert open(os.path.join(str(tmp_path / "unpacked"), m.name[2:]), "rb").read() == open(os.path.join(build, m.name[2:]), "rb").read()


def test_cli_xz_unxz_and_build_xz_unpack_xz(snaphash_mode, tmp_path):
    data = X.text(300000, 83) + X.rnd(70000, 84)
    (tmp_path / "in").write_bytes(data)
    subprocess.check_call([CLI, "xz", str(tmp_path / "in"), str(tmp_path / "out.xz"), "-B", "128"])
    z = (tmp_path / "out.xz").read_bytes()
    assert lzma.decompress(z) == data
    subprocess.check_call([CLI, "unxz", str(tmp_path / "out.xz"), str(tmp_path / "back")])
    assert (tmp_path / "back").read_bytes() == data
    subprocess.check_call([CLI, "xz", str(tmp_path / "in"), str(tmp_path / "out1m.xz")])
    assert lzma.decompress((tmp_path / "out1m.xz").read_bytes()) == data
    assert subprocess.run([CLI, "xz", str(tmp_path / "in"), str(tmp_path / "bad.xz"), "-B", "100"], capture_output=True).returncode == 2
    build, _ = trees.make_synthetic_tree(str(tmp_path), [0, 1, 1000, 65537, 200000])
    arc = str(tmp_path / "data.tar.xz")
    out = subprocess.run([CLI, "build-xz", build, arc], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    raw = open(arc, "rb").read()
    assert out.stdout.split() == [hashlib.sha512(raw).hexdigest(), arc]
    ypath = os.path.join(build, "DEBIAN", "hashes.yaml")
    subprocess.check_call([CLI, "unpack-xz", arc, str(tmp_path / "tree"), ypath])
    for dp, _, fs in os.walk(build):
        for f in fs:
            p = os.path.join(dp, f)
            rel = os.path.relpath(p, build)
            if not rel.startswith("DEBIAN"):
                assert open(os.path.join(str(tmp_path / "tree"), rel), "rb").read() == open(p, "rb").read(), rel
