"""data.tar.bz2 on the GPU: snaphash_bunzip2_buffer (blocks decoded side by side: the GPU bzip2 kernels under
FLAG_GPU_ONLY, host threads by default) and snaphash_tar_unpack_bz2 (ClickDeb.Unpack of a data.tar.bz2 with the
install-time Verify from the decoded bytes), in both configurations (conftest.py snaphash_mode).  The gz path of
tests/test_gpu_unpack.py is the yardstick: the same tar bytes must unpack and verify the same way."""
import bz2
import gzip
import io
import os
import tarfile

import pytest

from snappy_amd import Context, _lib, clickdeb, getHashes
from test_gpu_unpack import corpus, make_tree, tree_view

pytestmark = pytest.mark.gpu


def check_stats(c, mode, data, z):
    st = c.unpack_stats()
    assert st["tar_bytes"] == len(data) and st["gz_bytes"] == len(z), st
    if mode == "gpu_only":
        assert st["gpu_segments"] == st["segments"] and st["host_bytes"] == 0, st
    else:  # host threads, or the kernels where fewer than two cores are usable
        assert (st["gpu_segments"] == 0 and st["host_bytes"] == len(data)) or (st["gpu_segments"] == st["segments"] and st["host_bytes"] == 0), st
    return st


@pytest.mark.parametrize("kind", ["text", "binary", "random", "zeros"])
def test_bunzip2_matches_libbz2(snaphash_mode, kind):
    with Context(device=0) as c:
        for n, lv in ((1, 9), (4 << 20, 1), (4 << 20, 9)):
            data = corpus(kind, n, seed=n + lv)
            z = bz2.compress(data, lv)
            assert c.bunzip2_buffer(z) == data, (kind, n, lv)
            st = check_stats(c, snaphash_mode, data, z)
            assert st["segments"] >= 1
        z = bz2.compress(b"")
        assert c.bunzip2_buffer(z) == b""


def test_concatenated_streams_and_the_zeros_block(snaphash_mode):
    a, b, d = corpus("text", 900000, 1), corpus("random", 300000, 2), corpus("binary", 2 << 20, 3)
    with Context(device=0) as c:
        z = bz2.compress(a, 1) + bz2.compress(b, 5) + bz2.compress(b"", 3) + bz2.compress(d, 9)
        assert c.bunzip2_buffer(z) == a + b + d
        check_stats(c, snaphash_mode, a + b + d, z)
        zeros = bytes(43 << 20)  # one block that expands about 51x
        z = bz2.compress(zeros, 9)
        assert c.bunzip2_buffer(z) == zeros
        st = check_stats(c, snaphash_mode, zeros, z)
        assert st["segments"] == 1


@pytest.mark.kernels_only("256 MiB at full size, once")
def test_bunzip2_256_mib(snaphash_mode):
    data = corpus("text", 256 << 20, seed=4)
    z = bz2.compress(data, 9)
    with Context(device=0) as c:
        assert c.bunzip2_buffer(z) == data
        st = c.unpack_stats()
        assert st["gpu_segments"] == st["segments"] >= 250 and st["host_bytes"] == 0, st


def test_small_staging_forces_pieces(snaphash_mode):
    data = corpus("text", 12 << 20, seed=8) + corpus("random", 3 << 20, seed=9)
    z = bz2.compress(data, 9)
    with Context(device=0, staging_bytes=1 << 20) as c:
        assert c.bunzip2_buffer(z) == data
        check_stats(c, snaphash_mode, data, z)


def test_corrupt_stream_is_eformat_and_ctx_survives(snaphash_mode):
    data = corpus("text", 3 << 20, seed=10)
    z = bz2.compress(data, 9)
    with Context(device=0) as c:
        mid = bytearray(z)
        mid[len(mid) // 2] ^= 0x10
        for bad in (bytes(mid), z[: len(z) // 2], z + b"junk", b"BZh0" + z[4:], b"", b"BZh9" + bytes(40),
                    z + (0x314159265359).to_bytes(6, "big") * 50000):
            with pytest.raises(_lib.SnaphashError) as e:
                c.bunzip2_buffer(bad)
            assert e.value.code == _lib.EFORMAT
        assert c.bunzip2_buffer(z) == data


def tar_bytes(build):
    """The tree as tarfile writes it, the way tarCreate names members ("./<path>", DEBIAN left out)."""
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w", format=tarfile.GNU_FORMAT) as t:
        for name in sorted(os.listdir(build)):
            if name != "DEBIAN":
                t.add(os.path.join(build, name), arcname="./" + name)
    return buf.getvalue()


def test_unpack_bz2_matches_tarfile_and_the_gz_path(snaphash_mode, tmp_path):
    build = make_tree(str(tmp_path))
    raw = tar_bytes(build)
    arc_bz, arc_gz = tmp_path / "data.tar.bz2", tmp_path / "data.tar.gz"
    arc_bz.write_bytes(bz2.compress(raw, 9))
    arc_gz.write_bytes(gzip.compress(raw, 6))
    with Context(device=0) as c:
        mis, dig = c.tar_unpack_bz2(str(arc_bz), str(tmp_path / "bz"))
        assert mis is None
        import hashlib
        assert dig == hashlib.sha512(arc_bz.read_bytes()).digest()
        st = c.unpack_stats()
        assert st["members"] >= 10 and st["tar_bytes"] == len(raw)
        if snaphash_mode == "gpu_only":
            assert st["gpu_segments"] == st["segments"] and st["host_bytes"] == 0, st
        assert c.tar_unpack(str(arc_gz), str(tmp_path / "gz"))[0] is None
    assert tree_view(str(tmp_path / "bz")) == tree_view(str(tmp_path / "gz"))
    um = os.umask(0)
    os.umask(um)
    ref = tmp_path / "ref"
    with tarfile.open(str(arc_bz), "r:bz2") as t:
        for m in t.getmembers():
            p = os.path.join(ref, os.path.normpath(m.name))
            os.makedirs(os.path.dirname(p), exist_ok=True)
            if m.isdir():
                os.makedirs(p, exist_ok=True)
                os.chmod(p, m.mode & ~um)
            elif m.issym():
                os.symlink(m.linkname, p)
            else:
                with open(p, "wb") as f:
                    f.write(t.extractfile(m).read())
                os.chmod(p, m.mode & ~um)
    assert tree_view(str(tmp_path / "bz")) == tree_view(str(ref))


@pytest.fixture
def umask_022():
    old = os.umask(0o022)
    yield
    os.umask(old)


def _yaml_for(yaml, arc):
    """hashes.yaml with its archive-sha512 line naming `arc`."""
    import hashlib
    lines = yaml.split(b"\n")
    for i, ln in enumerate(lines):
        if ln.startswith(b"archive-sha512: "):
            lines[i] = b"archive-sha512: " + hashlib.sha512(open(arc, "rb").read()).hexdigest().encode()
    return b"\n".join(lines)


def test_unpack_bz2_verify_matches_the_gz_path(snaphash_mode, tmp_path, umask_022):
    build = make_tree(str(tmp_path))
    arc_gz = str(tmp_path / "data.tar.gz")
    with Context(device=0) as c:
        yaml, _ = c.tar_create(arc_gz, build, build + "/DEBIAN", with_hashes=True)
        arc_bz = str(tmp_path / "data.tar.bz2")
        with open(arc_bz, "wb") as f:
            f.write(bz2.compress(gzip.decompress(open(arc_gz, "rb").read()), 9))
        y_gz, y_bz = yaml, _yaml_for(yaml, arc_bz)
        assert c.tar_unpack(arc_gz, str(tmp_path / "g0"), y_gz)[0] is None
        assert c.tar_unpack_bz2(arc_bz, str(tmp_path / "b0"), y_bz)[0] is None
        lines = yaml.split(b"\n")
        idx = lines.index(b"- name: bin/run")
        for k, (what, fn) in enumerate([("sha512", lambda ln: ln[:-1] + (b"0" if ln[-1:] != b"0" else b"1")),
                                        ("size", lambda ln: ln + b"1"), ("mode", lambda ln: ln.replace(b"x", b"-", 1))]):
            j = next(i for i in range(idx, len(lines)) if lines[i].startswith(b"  %s: " % what.encode()))
            alt = b"\n".join(lines[:j] + [fn(lines[j])] + lines[j + 1:])
            mg, _ = c.tar_unpack(arc_gz, str(tmp_path / ("g%d" % (k + 1))), _yaml_for(alt, arc_gz))
            mb, _ = c.tar_unpack_bz2(arc_bz, str(tmp_path / ("b%d" % (k + 1))), _yaml_for(alt, arc_bz))
            assert mg is not None and mb == mg, (what, mg, mb)
        # the archive digest of the other file: both refuse it the same way
        mg, _ = c.tar_unpack(arc_gz, str(tmp_path / "ga"), y_bz)
        mb, _ = c.tar_unpack_bz2(arc_bz, str(tmp_path / "ba"), y_gz)
        assert mg is not None and mb == mg
        assert clickdeb.UnpackBz2(arc_bz, str(tmp_path / "cd"), y_bz, ctx=c) is None


def flip_digest(yaml, name):
    """hashes.yaml with the last hex digit of `name`'s sha512 changed."""
    lines = yaml.split(b"\n")
    k = next(j for j in range(lines.index(b"- name: " + name.encode()), len(lines)) if lines[j].startswith(b"  sha512: "))
    lines[k] = lines[k][:-1] + (b"0" if lines[k][-1:] != b"0" else b"1")
    return b"\n".join(lines)


def test_verify_reads_the_stream_two_pieces_left_in_hbm(snaphash_mode, tmp_path, umask_022):
    """The decoded stream's copy in HBM across pieces: more than 4 MiB of compressed bytes with the staging size of
    test_small_staging_forces_pieces take two pieces, so under FLAG_GPU_ONLY the second piece's blocks are written behind
    the first's while Verify's copy is kept (bunzip2_batch with a base that is not 0).  Level 1: a block is 100 000
    bytes, and runs in random bytes are too rare for RLE1 to change that.  Two pieces: a piece is never under 4 MiB
    (unbz2.inc, P in bunzip2_engine: max(staging, 4 MiB)), which the bounds on len(z) below rely on.  The copy in HBM is
    read back under FLAG_GPU_ONLY, where every member is hashed by the kernels; the default configuration hashes the
    members on host threads wherever 8 or more cores are usable, and checks the same digests from host memory."""
    from test_gpu_inflate_edges import tar_of
    files = {"r%d" % k: corpus("random", 1 << 20, seed=20 + k) for k in range(5)}
    files["notes"] = corpus("text", 3000, seed=30)
    raw = tar_of(files)
    z = bz2.compress(raw, 1)
    assert bz2.decompress(z) == raw and 4 << 20 < len(z) <= 8 << 20
    arc = str(tmp_path / "data.tar.bz2")
    with open(arc, "wb") as f:
        f.write(z)
    with Context(device=0, staging_bytes=1 << 20) as c:
        assert c.tar_unpack_bz2(arc, str(tmp_path / "plain"))[0] is None
        assert {k: (tmp_path / "plain" / k).read_bytes() for k in files} == files
        yaml = getHashes(str(tmp_path / "plain"), arc, c)
        assert c.tar_unpack_bz2(arc, str(tmp_path / "verified"), yaml)[0] is None
        st = check_stats(c, snaphash_mode, raw, z)
        assert st["members"] == len(files) and st["segments"] >= len(raw) // 100000, st
        if snaphash_mode == "gpu_only":
            assert st["gpu_segments"] == st["segments"] and st["host_bytes"] == 0, st
        mis, _ = c.tar_unpack_bz2(arc, str(tmp_path / "tampered"), flip_digest(yaml, "notes"))
        assert mis is not None and mis[1] == "notes", mis


def test_dotdot_member_is_econtent_and_stays_inside(snaphash_mode, tmp_path):
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w:bz2", format=tarfile.GNU_FORMAT) as t:
        for name, data in (("./ok", b"fine"), ("./a/../../escape", b"evil")):
            ti = tarfile.TarInfo(name)
            ti.size = len(data)
            t.addfile(ti, io.BytesIO(data))
    arc = tmp_path / "evil.tar.bz2"
    arc.write_bytes(buf.getvalue())
    target = tmp_path / "inside" / "dir"
    with Context(device=0) as c:
        with pytest.raises(_lib.SnaphashError) as e:
            c.tar_unpack_bz2(str(arc), str(target))
        assert e.value.code == _lib.ECONTENT
    assert not (tmp_path / "inside" / "escape").exists() and not (tmp_path / "escape").exists()
