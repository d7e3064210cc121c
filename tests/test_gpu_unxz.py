"""data.tar.xz on the GPU: snaphash_unxz_buffer (Blocks decoded side by side: lzma2_blocks_kernel under FLAG_GPU_ONLY,
host threads by default) and snaphash_tar_unpack_xz (ClickDeb.Unpack of a data.tar.xz with the install-time Verify from
the decoded bytes), in both configurations (conftest.py snaphash_mode), against liblzma through Python's lzma.  The gz
and bz2 paths are the yardstick for the unpack: the same tar bytes must unpack and verify the same way."""
import bz2
import gzip
import hashlib
import io
import lzma
import os
import subprocess
import tarfile

import pytest

import xz_cases as X
from snappy_amd import Context, _lib, clickdeb, getHashes
from test_gpu_bunzip2 import _yaml_for, flip_digest, tar_bytes, umask_022  # noqa: F401 (umask_022 is a fixture)
from test_gpu_inflate_edges import tar_of
from test_gpu_unpack import corpus, make_tree, tree_view

pytestmark = pytest.mark.gpu

GPU_BLOCK_MAX = 4 << 20  # kXzGpuBlockMax (xz_kernels.h)


def blocks_of(data, size):
    return [X.raw_lzma2(data[i:i + size]) for i in range(0, max(len(data), 1), size)]


def check_stats(c, mode, data, z, nblocks, host_bytes=0):
    st = c.unpack_stats()
    assert st["tar_bytes"] == len(data) and st["gz_bytes"] == len(z) and st["segments"] == nblocks, st
    if mode == "gpu_only":
        assert st["host_bytes"] == host_bytes and (host_bytes or st["gpu_segments"] == st["segments"]), st
    else:
        assert st["gpu_segments"] == 0 and st["host_bytes"] == len(data), st
    return st


@pytest.mark.parametrize("kind", ["text", "binary", "random", "zeros"])
def test_unxz_matches_liblzma(snaphash_mode, kind):
    with Context(device=0) as c:
        # (bytes, Block size): 1 byte in its one Block; 1 MiB in one Block; 4 MiB in 16 Blocks of 256 KiB
        for n, bs in ((1, 1), (1 << 20, 1 << 20), (4 << 20, 256 << 10)):
            data = corpus(kind, n, seed=n)
            z = X.xz_file(blocks_of(data, bs))
            assert lzma.decompress(z) == data
            assert c.unxz_buffer(z) == data, (kind, n)
            check_stats(c, snaphash_mode, data, z, (n + bs - 1) // bs)


def test_streams_checks_and_liblzmas_own_files(snaphash_mode):
    with Context(device=0) as c:
        for name, z, plain in X.container_cases():
            assert c.unxz_buffer(z) == plain, name
        t = corpus("text", 300000, 5)
        z = lzma.compress(t, format=lzma.FORMAT_XZ, check=lzma.CHECK_SHA256, preset=1)
        assert c.unxz_buffer(z) == t
        check_stats(c, snaphash_mode, t, z, 1)


def test_block_over_the_gpu_cap_goes_to_a_host_thread(snaphash_mode):
    big = bytes(GPU_BLOCK_MAX + 1)  # zeros: a long Block that costs the host decoder little
    small = corpus("text", 100000, 6)
    z = X.xz_file([X.raw_lzma2(small), X.raw_lzma2(big, dict_size=1 << 16), X.raw_lzma2(small)])
    with Context(device=0) as c:
        assert c.unxz_buffer(z) == small + big + small
        st = check_stats(c, snaphash_mode, small + big + small, z, 3, host_bytes=len(big))
        if snaphash_mode == "gpu_only":
            assert st["gpu_segments"] == 2


def test_bad_is_eformat_unsupported_is_einval_and_ctx_survives(snaphash_mode):
    t = corpus("text", 200000, 7)
    good = X.xz_file(blocks_of(t, 50000))
    with Context(device=0) as c:
        for name, z, _ in X.bad_cases():
            with pytest.raises(_lib.SnaphashError) as e:
                c.unxz_buffer(z)
            assert e.value.code == _lib.EFORMAT, name
        with pytest.raises(_lib.SnaphashError) as e:
            c.unxz_buffer(b"")
        assert e.value.code == _lib.EFORMAT
        for name, z in X.unsupported_cases():
            with pytest.raises(_lib.SnaphashError) as e:
                c.unxz_buffer(z)
            assert e.value.code == _lib.EINVAL, name
            if name != "check_id_2":
                assert "xz: unsupported filter 0x0" in str(e.value), str(e.value)
        assert c.unxz_buffer(good) == t


def _xz_of(raw):
    return X.xz_file(blocks_of(raw, 1 << 20), X.CHECK_CRC64)


def test_unpack_xz_matches_the_gz_and_bz2_paths(snaphash_mode, tmp_path):
    build = make_tree(str(tmp_path))
    raw = tar_bytes(build)
    arcs = {"xz": tmp_path / "data.tar.xz", "bz": tmp_path / "data.tar.bz2", "gz": tmp_path / "data.tar.gz"}
    arcs["xz"].write_bytes(_xz_of(raw))
    arcs["bz"].write_bytes(bz2.compress(raw, 9))
    arcs["gz"].write_bytes(gzip.compress(raw, 6))
    with Context(device=0) as c:
        mis, dig = c.tar_unpack_xz(str(arcs["xz"]), str(tmp_path / "xz"))
        assert mis is None and dig == hashlib.sha512(arcs["xz"].read_bytes()).digest()
        st = c.unpack_stats()
        assert st["members"] >= 10 and st["tar_bytes"] == len(raw) and st["segments"] == (len(raw) + (1 << 20) - 1) >> 20
        if snaphash_mode == "gpu_only":
            assert st["gpu_segments"] == st["segments"] and st["host_bytes"] == 0, st
        assert c.tar_unpack_bz2(str(arcs["bz"]), str(tmp_path / "bz"))[0] is None
        assert c.tar_unpack(str(arcs["gz"]), str(tmp_path / "gz"))[0] is None
    assert tree_view(str(tmp_path / "xz")) == tree_view(str(tmp_path / "gz")) == tree_view(str(tmp_path / "bz"))


def test_unpack_xz_verify_matches_the_gz_path(snaphash_mode, tmp_path, umask_022):
    build = make_tree(str(tmp_path))
    arc_gz = str(tmp_path / "data.tar.gz")
    with Context(device=0) as c:
        yaml, _ = c.tar_create(arc_gz, build, build + "/DEBIAN", with_hashes=True)
        arc_xz = str(tmp_path / "data.tar.xz")
        with open(arc_xz, "wb") as f:
            f.write(_xz_of(gzip.decompress(open(arc_gz, "rb").read())))
        y_gz, y_xz = yaml, _yaml_for(yaml, arc_xz)
        assert c.tar_unpack(arc_gz, str(tmp_path / "g0"), y_gz)[0] is None
        assert c.tar_unpack_xz(arc_xz, str(tmp_path / "x0"), y_xz)[0] is None
        lines = yaml.split(b"\n")
        idx = lines.index(b"- name: bin/run")
        for k, (what, fn) in enumerate([("sha512", lambda ln: ln[:-1] + (b"0" if ln[-1:] != b"0" else b"1")),
                                        ("size", lambda ln: ln + b"1"), ("mode", lambda ln: ln.replace(b"x", b"-", 1))]):
            j = next(i for i in range(idx, len(lines)) if lines[i].startswith(b"  %s: " % what.encode()))
            alt = b"\n".join(lines[:j] + [fn(lines[j])] + lines[j + 1:])
            mg, _ = c.tar_unpack(arc_gz, str(tmp_path / ("g%d" % (k + 1))), _yaml_for(alt, arc_gz))
            mx, _ = c.tar_unpack_xz(arc_xz, str(tmp_path / ("x%d" % (k + 1))), _yaml_for(alt, arc_xz))
            assert mg is not None and mx == mg, (what, mg, mx)
        mg, _ = c.tar_unpack(arc_gz, str(tmp_path / "ga"), y_xz)  # the archive digest of the other file
        mx, _ = c.tar_unpack_xz(arc_xz, str(tmp_path / "xa"), y_gz)
        assert mg is not None and mx == mg
        assert clickdeb.UnpackXz(arc_xz, str(tmp_path / "cd"), y_xz, ctx=c) is None


def test_verify_reads_a_host_block_between_kernel_blocks(snaphash_mode, tmp_path, umask_022):
    """The decoded stream's copy in HBM where its bytes come from both sides: three Blocks, the middle one over the
    kernel's cap (a host thread decodes it and its bytes are copied up between the two the kernel wrote in place), and
    members `a` and `big` that each lie across a Block boundary.  Verify hashes the members out of HBM under
    FLAG_GPU_ONLY; the default configuration decodes every Block on host threads and, wherever 8 or more cores are
    usable, hashes the members there too: it checks the same digests from host memory."""
    files = {"a": corpus("text", 100000, 11), "big": bytes(GPU_BLOCK_MAX + 4096), "c": corpus("text", 100000, 12)}
    raw = tar_of(files)
    cuts = [0, 65536, 65536 + GPU_BLOCK_MAX + 512, len(raw)]
    a0, big0 = 512, 512 + 100352 + 512  # where the members' bytes begin in the tar stream
    assert raw[a0:a0 + 100000] == files["a"] and a0 < cuts[1] < a0 + 100000
    assert raw[big0:big0 + 8] == bytes(8) and big0 < cuts[2] < big0 + len(files["big"]) and cuts[2] < len(raw) <= cuts[2] + GPU_BLOCK_MAX
    z = X.xz_file([X.raw_lzma2(raw[cuts[k]:cuts[k + 1]], dict_size=1 << 16) for k in range(3)], X.CHECK_CRC64)
    assert lzma.decompress(z) == raw
    arc = str(tmp_path / "data.tar.xz")
    with open(arc, "wb") as f:
        f.write(z)
    with Context(device=0) as c:
        assert c.tar_unpack_xz(arc, str(tmp_path / "plain"))[0] is None
        assert {k: (tmp_path / "plain" / k).read_bytes() for k in files} == files
        yaml = getHashes(str(tmp_path / "plain"), arc, c)
        assert c.tar_unpack_xz(arc, str(tmp_path / "verified"), yaml)[0] is None
        st = check_stats(c, snaphash_mode, raw, z, 3, host_bytes=cuts[2] - cuts[1])
        if snaphash_mode == "gpu_only":
            assert st["gpu_segments"] == 2, st
        for name in ("a", "big"):
            mis, _ = c.tar_unpack_xz(arc, str(tmp_path / ("tampered_" + name)), flip_digest(yaml, name))
            assert mis is not None and mis[1] == name, (name, mis)


def test_dotdot_member_is_econtent_and_stays_inside(snaphash_mode, tmp_path):
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w:xz", format=tarfile.GNU_FORMAT) as t:
        for name, data in (("./ok", b"fine"), ("./a/../../evil", b"evil")):
            ti = tarfile.TarInfo(name)
            ti.size = len(data)
            t.addfile(ti, io.BytesIO(data))
    arc = tmp_path / "evil.tar.xz"
    arc.write_bytes(buf.getvalue())
    with Context(device=0) as c:
        with pytest.raises(_lib.SnaphashError) as e:
            c.tar_unpack_xz(str(arc), str(tmp_path / "inside" / "dir"))
        assert e.value.code == _lib.ECONTENT
    assert not (tmp_path / "inside" / "evil").exists() and not (tmp_path / "evil").exists()


def test_cli_unxz_and_unpack_xz(snaphash_mode, tmp_path):
    from conftest import ROOT
    cli = os.path.join(ROOT, "snappy_amd", "bin", "snaphash")
    data = corpus("text", 500000, 8)
    (tmp_path / "in.xz").write_bytes(X.xz_file(blocks_of(data, 100000)))
    subprocess.check_call([cli, "unxz", str(tmp_path / "in.xz"), str(tmp_path / "out")])
    assert (tmp_path / "out").read_bytes() == data
    build = make_tree(str(tmp_path))
    (tmp_path / "data.tar.xz").write_bytes(_xz_of(tar_bytes(build)))
    subprocess.check_call([cli, "unpack-xz", str(tmp_path / "data.tar.xz"), str(tmp_path / "tree")])
    assert (tmp_path / "tree" / "bin" / "run").read_bytes() == (tmp_path / "build" / "bin" / "run").read_bytes()
