"""The .snap session on packages with .xz members (snaphash_snap_open_ex with SNAPHASH_SNAP_XZ, snappy_amd/csrc/snap.inc):
every form of tests/snap_xz_cases.py audited, unpacked with the install-time Verify and read member by member, what the
session keeps whatever the codec (one decode a tar, the stream left in HBM and copied up again after another decode, the
archive digest, the unpack statistics), who took the Blocks' Checks, and every refusal and way of tampering the audit must
name -- in both configurations, with the same verdict in each (every test states the verdict it expects, so the two runs
cannot differ).  The oracle is lzma / tarfile / hashlib and the oracle's hashes.yaml; the member lookup by itself is in
tests/test_snap_xz_host.py."""
import ctypes
import hashlib
import io
import os
import subprocess
import tarfile

import pytest

import snap_cases as S
import snap_xz_cases as X
from conftest import ROOT

pytestmark = pytest.mark.gpu

EINVAL, EFORMAT = -1, -9
META = b"name: hello\nversion: 1.0\n"


@pytest.fixture(scope="module")
def pk(tmp_path_factory, oracle, built_lib):
    """The tree, its tar stream, and per form the .xz member's bytes and the oracle's hashes.yaml over it."""
    from snappy_amd import Context, _lib
    tmp = str(tmp_path_factory.mktemp("snapxz"))
    old = os.umask(0o022)
    build = S.make_tree(tmp)
    tar = S.tar_of(build)
    assert len(tar) > X.BLOCK
    forms = {}
    with Context(flags=_lib.FLAG_GPU_ONLY) as c:
        for form in X.FORMS:
            data = X.compress(form, tar, ctx=c)
            forms[form] = {"data": data, "yaml": S.hashes_yaml(oracle, build, data, tmp)}
    gz = S.gz(tar)
    forms["gz"] = {"data": gz, "yaml": S.hashes_yaml(oracle, build, gz, tmp)}
    ref = os.path.join(tmp, "ref")
    S.extract_reference(tar, ref)
    with tarfile.open(fileobj=io.BytesIO(tar)) as t:
        members = len(t.getmembers())
    yield {"tmp": tmp, "build": build, "tar": tar, "forms": forms, "oracle": oracle, "ref": S.tree_listing(ref), "members": members}
    os.umask(old)


@pytest.fixture(scope="module")
def _ctxs():
    made = {}
    yield made
    for c in made.values():
        c.close()


@pytest.fixture
def sctx(snaphash_mode, built_lib, _ctxs):
    """A context in the configuration of this run (the flags come from the snaphash_mode fixture), one per mode."""
    from snappy_amd import Context
    if snaphash_mode not in _ctxs:
        _ctxs[snaphash_mode] = Context()
    return _ctxs[snaphash_mode]


_n = [0]


def snap_of(pk, form, yaml="own", data=None, control="gz", data_name=None):
    """A package whose data member is the form's (or `data`), its control member gzip or .xz."""
    f = pk["forms"][form]
    _n[0] += 1
    path = os.path.join(pk["tmp"], "x%d.snap" % _n[0])
    ctl = X.control_tar(f["yaml"] if yaml == "own" else yaml)
    X.write_snap(path, ("control.tar.gz", S.gz(ctl)) if control == "gz" else ("control.tar.xz", X.xz(ctl)),
                 (data_name or ("data.tar.gz" if form == "gz" else "data.tar.xz"), f["data"] if data is None else data))
    return path


def blocks_of(pk):
    return -(-len(pk["tar"]) // X.BLOCK)


def hold_session(sctx, pk, path, form, tmp_path, control_name="control.tar.gz"):
    """what every readable package must give; -> the session's statistics at the end"""
    f = pk["forms"][form]
    with sctx.snap_open(path, xz=True) as s:
        assert [m[0] for m in s.members()] == ["debian-binary", control_name, "data.tar.gz" if form == "gz" else "data.tar.xz"]
        verdict, dig = s.audit()
        assert verdict is None
        assert dig == hashlib.sha512(f["data"]).digest()
        us = sctx.unpack_stats()  # of the data member's decode
        assert us["gz_bytes"] == len(f["data"]) and us["tar_bytes"] == len(pk["tar"]) and us["members"] == pk["members"]
        target = str(tmp_path / "out")
        os.mkdir(target)
        verdict, dig = s.unpack(target, verify=True)
        assert verdict is None and dig == hashlib.sha512(f["data"]).digest()
        assert S.tree_listing(target) == pk["ref"]
        assert sctx.verify(target, f["yaml"]) is None
        assert s.meta_member("package.yaml") == META
        assert s.control_member("manifest") == b"{}\n"
        assert s.control_member("hashes.yaml") == f["yaml"]
        assert s.control_member("nothing") is None and s.meta_member("nothing") is None
        st = s.stats()
        assert st["data_decodes"] == 1 and st["control_decodes"] == 1
        return st


@pytest.mark.parametrize("form", X.FORMS)
def test_audit_unpack_members(sctx, snaphash_mode, pk, form, tmp_path):
    hold_session(sctx, pk, snap_of(pk, form), form, tmp_path)


@pytest.mark.parametrize("form", ["gz", "xz1", "own"])
def test_control_tar_xz(sctx, snaphash_mode, pk, form, tmp_path):
    """control.tar.xz beside a data.tar.gz, and beside a data.tar.xz: the control member takes the same switch."""
    hold_session(sctx, pk, snap_of(pk, form, control="xz"), form, tmp_path, control_name="control.tar.xz")


@pytest.mark.parametrize("form", list(X.OWN_FORMS))
def test_who_takes_the_checks_of_own_blocks(sctx, snaphash_mode, pk, form):
    """The library's own multi-Block members: under SNAPHASH_FLAG_GPU_ONLY every Block goes through lzma2_blocks_kernel and
    its Check through the CRC-64 kernel; planned, Blocks and Checks stay on host threads."""
    nb = blocks_of(pk)
    assert nb >= 2
    with sctx.snap_open(snap_of(pk, form), xz=True) as s:
        st0 = s.stats()
        assert st0["data_decodes"] == 0 and st0["device_crc_ranges"] == 0 and st0["host_crc_ranges"] == 0  # open decodes nothing
        assert s.meta_member("package.yaml") == META   # the data member alone
        st = s.stats()
        assert st["data_decodes"] == 1 and st["control_decodes"] == 0
        if snaphash_mode == "gpu_only":
            assert (st["device_crc_ranges"], st["host_crc_ranges"]) == (nb, 0) and st["device_crc_ms"] > 0
        else:
            assert (st["device_crc_ranges"], st["host_crc_ranges"]) == (0, nb)
        assert s.audit()[0] is None
        us = sctx.unpack_stats()
        assert us["segments"] == nb and us["gpu_segments"] == (nb if snaphash_mode == "gpu_only" else 0)
        fs = sctx.xz_filter_stats()  # of the data member's decode, the last .xz call of the ctx
        if form == "own-x86-L1":
            assert fs["filter"] == 4 and (fs["device_blocks"], fs["host_blocks"]) == ((nb, 0) if snaphash_mode == "gpu_only" else (0, nb))
        # the data member's own counts are not taken again by what follows
        after = s.stats()
        assert after["data_decodes"] == 1 and after["device_crc_ranges"] == st["device_crc_ranges"]
        assert after["host_crc_ranges"] > st["host_crc_ranges"]   # control.tar.gz's gzip member, on a host thread in both


@pytest.mark.parametrize("form", ["xz1", "own"])
def test_meta_member_then_unpack_decodes_once(sctx, snaphash_mode, pk, form, tmp_path):
    with sctx.snap_open(snap_of(pk, form, control="xz"), xz=True) as s:
        assert s.stats()["data_decodes"] == 0
        assert s.meta_member("package.yaml") is not None
        assert s.stats()["data_decodes"] == 1 and s.stats()["control_decodes"] == 0
        # control.tar.xz is decoded in between and takes the buffer the data.tar stream was left in: the Verify and the audit
        # hash the stream in HBM, so it has to be copied up again -- and is not decoded again
        assert s.unpack(str(tmp_path), verify=True)[0] is None
        assert s.audit()[0] is None
        # another session's decode on the same ctx in between
        with sctx.snap_open(snap_of(pk, "xzsha"), xz=True) as other:
            assert other.audit()[0] is None
        assert s.audit()[0] is None
        st = s.stats()
        assert st["data_decodes"] == 1 and st["control_decodes"] == 1


def test_without_the_flag_xz_is_refused(sctx, snaphash_mode, pk):
    from snappy_amd import SnaphashError, _lib
    opens = [lambda p: sctx.snap_open(p), lambda p: _lib.Snap(sctx, p, _opt=_lib.SnapOpenOptions(0, 0)),
             lambda p: _lib.Snap(sctx, p, _opt=_lib.SnapOpenOptions(ctypes.sizeof(_lib.SnapOpenOptions), 0))]
    for form in ("xz1", "own"):
        path = snap_of(pk, form)
        for op in opens:
            with op(path) as s:
                for call in (lambda: s.meta_member("package.yaml"), s.audit):
                    with pytest.raises(SnaphashError) as e:
                        call()
                    assert e.value.code == EINVAL and "Can not handle data.tar.xz" in str(e.value)
                assert s.control_member("manifest") == b"{}\n"  # the other tar is still read
                assert s.stats()["data_decodes"] == 0
    with sctx.snap_open(snap_of(pk, "gz", control="xz")) as s:
        with pytest.raises(SnaphashError) as e:
            s.control_member("manifest")
        assert e.value.code == EINVAL and "Can not handle control.tar.xz" in str(e.value)
        assert s.meta_member("package.yaml") == META


def test_open_options(sctx, snaphash_mode, pk):
    from snappy_amd import SnaphashError, _lib
    path = snap_of(pk, "xz1")
    size = ctypes.sizeof(_lib.SnapOpenOptions)
    for opt in (_lib.SnapOpenOptions(size, 2), _lib.SnapOpenOptions(size, _lib.SNAP_XZ | 0x80000000), _lib.SnapOpenOptions(size - 1, _lib.SNAP_XZ),
                _lib.SnapOpenOptions(4, _lib.SNAP_XZ), _lib.SnapOpenOptions(0, _lib.SNAP_XZ)):
        with pytest.raises(SnaphashError) as e:
            _lib.Snap(sctx, path, _opt=opt)
        assert e.value.code == EINVAL
    # a larger struct_size is a newer caller's
    with _lib.Snap(sctx, path, _opt=_lib.SnapOpenOptions(size + 8, _lib.SNAP_XZ)) as s:
        assert s.meta_member("package.yaml") == META


def test_unsupported_chain_is_remembered(sctx, snaphash_mode, pk):
    from snappy_amd import SnaphashError
    with sctx.snap_open(snap_of(pk, "xz1", data=X.delta(pk["tar"])), xz=True) as s:
        for _ in range(2):  # the failure is the session's: the second call answers what the first did
            with pytest.raises(SnaphashError) as e:
                s.audit()
            assert e.value.code == EINVAL and "xz: unsupported filter 0x03" in str(e.value)
        assert s.stats()["data_decodes"] == 1
        assert s.control_member("manifest") == b"{}\n"


@pytest.mark.parametrize("form", ["xz1", "own"])
@pytest.mark.parametrize("where", ["body", "check", "index"])
def test_one_flipped_byte(sctx, snaphash_mode, pk, form, where):
    from snappy_amd import SnaphashError
    good = pk["forms"][form]["data"]
    data = X.flip(good, X.layout(good)[where])
    assert len(data) == len(good)
    with sctx.snap_open(snap_of(pk, form, data=data), xz=True) as s:
        with pytest.raises(SnaphashError) as e:
            s.audit()
        assert e.value.code == EFORMAT, str(e.value)
        assert s.control_member("hashes.yaml") == pk["forms"][form]["yaml"]


def test_tampered_yaml_and_member(sctx, snaphash_mode, pk):
    # archive-sha512 of other bytes: the yaml of another form's member
    with sctx.snap_open(snap_of(pk, "own", yaml=pk["forms"]["xz1"]["yaml"]), xz=True) as s:
        assert s.audit()[0] == (6, "archive-sha512")
    # one byte of the 70 000-byte member flipped BEFORE the compression: every Check and archive-sha512 (the yaml is the
    # oracle's over the new member and the unchanged tree) agree, the record's digest does not
    with open(os.path.join(pk["build"], S.BIG_NAME), "rb") as f:
        needle = f.read()[40000:40032]
    at = pk["tar"].find(needle)
    assert at > 0
    for data in (X.xz(X.flip(pk["tar"], at + 7)), sctx.xz_buffer(X.flip(pk["tar"], at + 7), block_size=X.BLOCK)):
        yaml = S.hashes_yaml(pk["oracle"], pk["build"], data, pk["tmp"])
        with sctx.snap_open(snap_of(pk, "xz1", yaml=yaml, data=data), xz=True) as s:
            assert s.audit()[0] == (4, S.BIG_NAME)


def test_clickdeb_mirror(sctx, snaphash_mode, pk, tmp_path):
    from snappy_amd import SnaphashError
    from snappy_amd.clickdeb import ClickDeb
    path = snap_of(pk, "own-x86-L1")
    with ClickDeb.open(path, ctx=sctx, xz=True) as d:
        assert d.meta_member("package.yaml") == META
        assert d.audit() is None
        assert d.unpack(str(tmp_path)) is None
        assert d.stats()["data_decodes"] == 1
    with ClickDeb.open(path, ctx=sctx) as d:
        with pytest.raises(SnaphashError) as e:
            d.audit()
        assert e.value.code == EINVAL


@pytest.mark.kernels_only("the command-line tool names its own flags")
def test_cli_snap_verbs_with_x(pk, tmp_path):
    cli = os.path.join(ROOT, "snappy_amd", "bin", "snaphash")
    good = snap_of(pk, "own")
    r = subprocess.run([cli, "-g", "-s", "snap", "-x", "audit", good], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "OK\n", r.stderr
    assert "CRCs: %d on the device" % blocks_of(pk) in r.stderr
    r = subprocess.run([cli, "snap", "-x", "unpack", str(tmp_path), good], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "OK\n", r.stderr
    assert os.path.getsize(str(tmp_path / S.BIG_NAME)) == S.BIG
    r = subprocess.run([cli, "snap", "-x", "cat-meta", "package.yaml", good], capture_output=True)
    assert r.returncode == 0 and r.stdout == META
    r = subprocess.run([cli, "snap", "audit", good], capture_output=True, text=True)
    assert r.returncode == 2 and "Can not handle data.tar.xz" in r.stderr
