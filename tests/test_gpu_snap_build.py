"""snaphash_snap_build (snappy_amd/csrc/snapbuild.inc) through ClickDeb.create(path).build(dir): the package written from
one read of the tree, held against tarCreate of the same tree, hashlib, the oracle's hashes.yaml, Python's gzip and
tarfile, and the install side's own audit and unpack -- without and with the self-check (SNAPHASH_BUILD_CHECK), which must
not change a byte.  In both configurations; every test states what it expects, so the two runs cannot differ."""
import gzip
import hashlib
import io
import os
import shutil
import subprocess
import tarfile

import pytest

import snap_cases as S
import trees
from conftest import ROOT
from deflate_check_streams import payload

pytestmark = pytest.mark.gpu

EIO, EMODE = -3, -5
MTIME = 1445212800
NAMES = ["debian-binary", "_click-binary", "control.tar.gz", "data.tar.gz"]
SIZES = [0, 1, 111, 127, 128, 129, 1000, 4096, 65536, 65537, 100000, 3, 77, 5000, 64, 8, 16]  # + the stand-in make_synthetic_tree wants


def make_tree(root, control=b"Package: hello\nVersion: 1.0\n"):
    """a synthetic tree of tests/trees.py (incompressible members: stored chunks), one 200 KiB text file (four chunks that
    shrink), a symlink, and DEBIAN/ with control and manifest"""
    build, _ = trees.make_synthetic_tree(root, SIZES + [1])
    trees._write(os.path.join(build, "big.txt"), payload(200 * 1024, 3), 0o644)
    os.symlink("big.txt", os.path.join(build, "link"))
    os.makedirs(os.path.join(build, "DEBIAN"), mode=0o755)
    os.chmod(os.path.join(build, "DEBIAN"), 0o755)
    trees._write(os.path.join(build, "DEBIAN", "control"), control, 0o644)
    trees._write(os.path.join(build, "DEBIAN", "manifest"), b"{}\n", 0o644)
    return build


@pytest.fixture(scope="module")
def _ctxs():
    made = {}
    yield made
    for c in made.values():
        c.close()


@pytest.fixture
def sctx(snaphash_mode, built_lib, _ctxs):
    from snappy_amd import Context
    if snaphash_mode not in _ctxs:
        _ctxs[snaphash_mode] = Context()
    return _ctxs[snaphash_mode]


@pytest.fixture
def umask022():
    old = os.umask(0o022)
    yield
    os.umask(old)


def member_bytes(snap, members, name):
    blob = open(snap, "rb").read()
    off, size = {m[0]: (m[1], m[2]) for m in members}[name]
    return blob[off:off + size]


def hold_package(sctx, oracle, build, snap, w, tmp_path, tag):
    """everything the issue asks of a built package; -> the file's bytes"""
    from snappy_amd.clickdeb import ClickDeb
    blob = open(snap, "rb").read()
    assert hashlib.sha512(blob).digest() == w.snap_digest
    assert w.build_stats["snap_bytes"] == len(blob)
    ref_tar = str(tmp_path / ("ref-%s.tar.gz" % tag))
    ref_digest = sctx.tar_create(ref_tar, build, build + "/DEBIAN", with_hashes=True)[1]
    with ClickDeb.open(snap, ctx=sctx) as d:
        mem = d.members()
        assert [m[0] for m in mem] == NAMES
        assert member_bytes(snap, mem, "debian-binary") == b"2.0\n" and member_bytes(snap, mem, "_click-binary") == b"0.4\n"
        data = member_bytes(snap, mem, "data.tar.gz")
        assert data == open(ref_tar, "rb").read(), "the data member is not what tarCreate writes for the tree"
        assert hashlib.sha512(data).digest() == w.archive_digest == ref_digest
        assert w.build_stats["tar_bytes"] >= 4 * 65536 and w.build_stats["data_bytes"] == len(data)
        want_yaml = oracle.hashes_yaml(build, ref_tar)
        assert d.control_member("hashes.yaml") == want_yaml
        assert open(os.path.join(build, "DEBIAN", "hashes.yaml"), "rb").read() == want_yaml
        assert os.stat(os.path.join(build, "DEBIAN", "hashes.yaml")).st_mode & 0o777 == 0o644
        ctl = member_bytes(snap, mem, "control.tar.gz")
        with tarfile.open(fileobj=io.BytesIO(gzip.decompress(ctl))) as t:
            assert sorted(m.name for m in t.getmembers()) == ["./control", "./hashes.yaml", "./manifest"]
            assert t.extractfile("./hashes.yaml").read() == want_yaml
        assert d.audit() is None
        target = str(tmp_path / ("out-%s" % tag))
        os.mkdir(target)
        assert d.unpack(target, verify=True) is None
        want = S.tree_listing(build)
        want = {k: v for k, v in want.items() if k != "DEBIAN" and not k.startswith("DEBIAN/")}
        assert S.tree_listing(target) == want
    return blob


def test_build_and_read_back(sctx, snaphash_mode, oracle, tmp_path, umask022):
    from snappy_amd.clickdeb import ClickDeb
    build = make_tree(str(tmp_path))
    snap, snap2 = str(tmp_path / "hello.snap"), str(tmp_path / "checked.snap")
    yaml_path = os.path.join(build, "DEBIAN", "hashes.yaml")
    # "the same mtime" is two: the ar members' (given) and that of DEBIAN/hashes.yaml, which every build rewrites and
    # control.tar.gz carries in whole seconds.  The pair of builds (a few tens of ms) is taken again if a second ticked between them.
    for attempt in range(4):
        w = ClickDeb.create(snap, ctx=sctx).build(build, mtime=MTIME)
        second = int(os.stat(yaml_path).st_mtime)
        # the same with the self-check: every chunk of both tars walked on the GPU, not a byte different
        w2 = ClickDeb.create(snap2, ctx=sctx).build(build, check=True, mtime=MTIME)
        if int(os.stat(yaml_path).st_mtime) == second:
            break
    else:
        pytest.fail("four pairs of builds each straddled a second")
    assert w.build_stats["check_chunks"] == 0
    plain = hold_package(sctx, oracle, build, snap, w, tmp_path, "plain")
    assert not os.path.exists(snap + ".data.tar.gz") and not os.path.exists(snap + ".control.tar.gz")
    checked = hold_package(sctx, oracle, build, snap2, w2, tmp_path, "checked")
    assert checked == plain
    tar_chunks = (w2.build_stats["tar_bytes"] + 65535) // 65536
    assert w2.build_stats["check_chunks"] == tar_chunks + 1  # the data member's, and the one chunk of control.tar.gz
    assert w2.snap_digest == w.snap_digest and w2.archive_digest == w.archive_digest
    h = plain[8:68]
    assert h[:16] == b"debian-binary   " and h[16:28] == b"%-12d" % MTIME and h[40:48] == b"100644  "


def test_padding_odd_and_even_control(sctx, snaphash_mode, oracle, tmp_path, umask022):
    from snappy_amd.clickdeb import ClickDeb
    seen = {}
    for k in range(12):
        if len(seen) == 2:
            break
        root = tmp_path / ("t%d" % k)
        root.mkdir()
        build = make_tree(str(root), control=b"Package: hello\nVersion: 1.0\nDescription: " + bytes(65 + (7 * j) % 26 for j in range(k)) + b"\n")
        snap = str(root / "p.snap")
        ClickDeb.create(snap, ctx=sctx).build(build, check=bool(k & 1), mtime=MTIME)
        with ClickDeb.open(snap, ctx=sctx) as d:
            mem = {m[0]: m for m in d.members()}
            parity = mem["control.tar.gz"][2] % 2
            assert mem["data.tar.gz"][1] % 2 == 0
            assert mem["data.tar.gz"][1] == mem["control.tar.gz"][1] + mem["control.tar.gz"][2] + parity + 60
            if parity not in seen:
                assert d.audit() is None
            seen[parity] = k
        assert os.path.getsize(snap) % 2 == 0
    assert set(seen) == {0, 1}, "control.tar.gz never had both an odd and an even size"


def test_no_hashes(sctx, snaphash_mode, tmp_path, umask022):
    from snappy_amd.clickdeb import ClickDeb
    build = make_tree(str(tmp_path))
    snap = str(tmp_path / "nohashes.snap")
    w = ClickDeb.create(snap, ctx=sctx).build(build, hashes=False, mtime=MTIME)
    assert not os.path.exists(os.path.join(build, "DEBIAN", "hashes.yaml"))
    with ClickDeb.open(snap, ctx=sctx) as d:
        mem = d.members()
        assert [m[0] for m in mem] == NAMES
        assert d.control_member("hashes.yaml") is None and d.control_member("manifest") == b"{}\n"
        assert d.audit() == (1, "hashes.yaml")
        assert hashlib.sha512(member_bytes(snap, mem, "data.tar.gz")).digest() == w.archive_digest


def test_failures_leave_no_file(sctx, snaphash_mode, tmp_path, umask022):
    from snappy_amd import SnaphashError
    from snappy_amd.clickdeb import ClickDeb

    def refused(build, snap, code, **kw):
        with pytest.raises(SnaphashError) as e:
            ClickDeb.create(snap, ctx=sctx).build(build, mtime=MTIME, **kw)
        assert e.value.code == code, str(e.value)
        assert not os.path.exists(snap)
        assert not os.path.exists(snap + ".data.tar.gz") and not os.path.exists(snap + ".control.tar.gz")

    (tmp_path / "a").mkdir()
    build = make_tree(str(tmp_path / "a"))
    shutil.rmtree(os.path.join(build, "DEBIAN"))
    refused(build, str(tmp_path / "no-debian.snap"), EIO)
    refused(build, str(tmp_path / "no-debian-nil.snap"), EIO, hashes=False)
    (tmp_path / "b").mkdir()
    build = make_tree(str(tmp_path / "b"))
    os.mkfifo(os.path.join(build, "fifo"))
    refused(build, str(tmp_path / "fifo.snap"), EMODE, check=True)
    (tmp_path / "c").mkdir()
    build = make_tree(str(tmp_path / "c"))
    refused(build, str(tmp_path / "missing" / "p.snap"), EIO)
    # and the tree is still good for a build
    snap = str(tmp_path / "after.snap")
    ClickDeb.create(snap, ctx=sctx).build(build, mtime=MTIME)
    with ClickDeb.open(snap, ctx=sctx) as d:
        assert d.audit() is None


@pytest.mark.kernels_only("one round trip through the command-line tool")
def test_cli_snap_build_then_audit(tmp_path, umask022):
    cli = os.path.join(ROOT, "snappy_amd", "bin", "snaphash")
    build = make_tree(str(tmp_path))
    snap = str(tmp_path / "cli.snap")
    r = subprocess.run([cli, "-s", "snap", "build", "-c", build, snap], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split()[0] == hashlib.sha512(open(snap, "rb").read()).hexdigest()
    assert "self-check:" in r.stderr and "self-check: 0 chunks" not in r.stderr
    r = subprocess.run([cli, "snap", "audit", snap], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stderr
    r = subprocess.run([cli, "snap", "build", build, str(tmp_path / "missing" / "x.snap")], capture_output=True, text=True)
    assert r.returncode == 2 and not os.path.exists(str(tmp_path / "missing"))
