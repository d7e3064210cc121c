"""The .snap session (snappy_amd/csrc/snap.inc) on packages built in Python (tests/snap_cases.py): audit, unpack with the
install-time Verify, ControlMember / MetaMember, one decode per tar and session, ar's padding both ways, "last member
wins", and every way of tampering the audit must name -- in both configurations, with the same verdict in each (every test
states the verdict it expects, so the two runs cannot differ).  The oracle is tarfile / gzip / bz2 / hashlib and the
oracle's hashes.yaml; the container's parser and the audit's comparison by themselves are in tests/test_snap_host.py."""
import gzip
import os
import subprocess

import pytest

import snap_cases as S
from conftest import ROOT

pytestmark = pytest.mark.gpu

FORMS = ["pygz", "libgz", "bz2", "gz2"]
EINVAL, EFORMAT, ECONTENT = -1, -9, -10


@pytest.fixture(scope="module")
def pk(tmp_path_factory, oracle, built_lib):
    """The tree, and per data.tar form the member's bytes, the tar stream behind it and the oracle's hashes.yaml."""
    from snappy_amd import Context, _lib
    tmp = str(tmp_path_factory.mktemp("snap"))
    old = os.umask(0o022)
    build = S.make_tree(tmp)
    tar = S.tar_of(build)
    forms = {}
    with Context(flags=_lib.FLAG_GPU_ONLY) as c:
        for form in FORMS + ["stored"]:
            name, data = S.compress(form, tar, ctx=c, build=build, tmp=tmp)
            forms[form] = {"name": name, "data": data, "tar": gzip.decompress(data) if form == "libgz" else tar,
                           "yaml": S.hashes_yaml(oracle, build, data, tmp)}
    yield {"tmp": tmp, "build": build, "tar": tar, "forms": forms, "oracle": oracle}
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


def snap_of(pk, form, yaml="own", data=None, parity=None, lead=()):
    f = pk["forms"][form]
    _n[0] += 1
    path = os.path.join(pk["tmp"], "p%d.snap" % _n[0])
    S.write_snap(path, f["name"], f["data"] if data is None else data, f["yaml"] if yaml == "own" else yaml, parity, lead)
    return path


@pytest.mark.parametrize("form", FORMS)
def test_audit_unpack_members(sctx, snaphash_mode, pk, form, tmp_path):
    f = pk["forms"][form]
    with sctx.snap_open(snap_of(pk, form)) as s:
        assert [m[0] for m in s.members()] == ["debian-binary", "control.tar.gz", f["name"]]
        verdict, dig = s.audit()
        assert verdict is None
        import hashlib
        assert dig == hashlib.sha512(f["data"]).digest()
        target = str(tmp_path / "out")
        os.mkdir(target)
        assert s.unpack(target, verify=True)[0] is None
        ref = str(tmp_path / "ref")
        S.extract_reference(f["tar"], ref)
        assert S.tree_listing(target) == S.tree_listing(ref)
        assert sctx.verify(target, f["yaml"]) is None
        assert s.meta_member("package.yaml") == b"name: hello\nversion: 1.0\n"
        assert s.control_member("manifest") == b"{}\n"
        assert s.control_member("hashes.yaml") == f["yaml"]
        assert s.control_member("nothing") is None and s.meta_member("nothing") is None
        st = s.stats()
        assert st["data_decodes"] == 1 and st["control_decodes"] == 1
        # where the CRCs of the decodes were taken: on the device under SNAPHASH_FLAG_GPU_ONLY, on host threads otherwise
        if snaphash_mode == "gpu_only":
            assert st["device_crc_ranges"] >= (2 if form == "gz2" else 1)
        else:
            assert st["device_crc_ranges"] == 0 and st["host_crc_ranges"] >= 2


@pytest.mark.parametrize("form", ["pygz", "bz2"])
def test_meta_member_then_unpack_decodes_once(sctx, snaphash_mode, pk, form, tmp_path):
    with sctx.snap_open(snap_of(pk, form)) as s:
        assert s.stats()["data_decodes"] == 0  # open decodes nothing
        assert s.meta_member("package.yaml") is not None
        assert s.stats() ["data_decodes"] == 1 and s.stats()["control_decodes"] == 0
        # control.tar.gz is decoded in between and may take the buffer the data.tar stream was left in
        assert s.unpack(str(tmp_path), verify=True)[0] is None
        assert s.audit()[0] is None
        st = s.stats()
        assert st["data_decodes"] == 1 and st["control_decodes"] == 1


def test_control_length_odd_and_even(sctx, snaphash_mode, pk):
    seen = set()
    for parity in (0, 1):
        path = snap_of(pk, "pygz", parity=parity)
        with sctx.snap_open(path) as s:
            mem = {m[0]: m for m in s.members()}
            assert mem["control.tar.gz"][2] % 2 == parity
            assert mem["data.tar.gz"][1] % 2 == 0
            seen.add(mem["control.tar.gz"][2] % 2)
            assert s.audit()[0] is None
            assert s.control_member("hashes.yaml") == pk["forms"]["pygz"]["yaml"]
    assert seen == {0, 1}


STALE = [("meta/package.yaml", b"name: stale\n"), (S.BIG_NAME, b"stale")]


def test_last_member_of_a_name_wins(sctx, snaphash_mode, pk, tmp_path):
    tar = S.tar_of(pk["build"], extra_first=STALE)
    data = S.gz(tar)
    yaml = S.hashes_yaml(pk["oracle"], pk["build"], data, pk["tmp"])
    with sctx.snap_open(snap_of(pk, "pygz", yaml=yaml, data=data)) as s:
        assert s.meta_member("package.yaml") == b"name: hello\nversion: 1.0\n"
        assert s.audit()[0] is None
        assert s.unpack(str(tmp_path), verify=True)[0] is None
        with open(str(tmp_path / S.BIG_NAME), "rb") as f:
            assert len(f.read()) == S.BIG


def test_earlier_member_of_another_mode(sctx, snaphash_mode, pk, tmp_path):
    """The audit reads the tar headers, and the last member's is the one it holds a record against.  An unpack is the
    reference's UnpackTar: the second os.OpenFile(O_CREATE|O_TRUNC, mode) of a path finds the file there and leaves the
    mode the FIRST member created it with (helpers/helpers.go:132), so Verify on the tree names the mode."""
    data = S.gz(S.tar_of(pk["build"], extra_first=STALE, extra_mode=0o600))
    yaml = S.hashes_yaml(pk["oracle"], pk["build"], data, pk["tmp"])
    with sctx.snap_open(snap_of(pk, "pygz", yaml=yaml, data=data)) as s:
        assert s.audit()[0] is None
        assert s.unpack(str(tmp_path), verify=True)[0] == (5, S.BIG_NAME)
        with open(str(tmp_path / S.BIG_NAME), "rb") as f:
            assert len(f.read()) == S.BIG  # the content is the last member's all the same


def _flip_in_big(pk, blob):
    """One byte of the 70 000-byte member flipped in a byte string that holds the member verbatim."""
    with open(os.path.join(pk["build"], S.BIG_NAME), "rb") as f:
        needle = f.read()[40000:40032]
    at = blob.find(needle)
    assert at > 0 and blob.find(needle, at + 1) < 0
    return blob[:at + 7] + bytes([blob[at + 7] ^ 0x20]) + blob[at + 8:]


def test_tamper_member_byte_trailer_fixed(sctx, snaphash_mode, pk):
    """Re-compressed after the flip: CRC-32, ISIZE and archive-sha512 (the yaml is the oracle's over the new archive) all
    agree, the member's digest does not."""
    data = S.gz(_flip_in_big(pk, pk["tar"]))
    yaml = S.hashes_yaml(pk["oracle"], pk["build"], data, pk["tmp"])
    with sctx.snap_open(snap_of(pk, "pygz", yaml=yaml, data=data)) as s:
        assert s.audit()[0] == (4, S.BIG_NAME)


def test_tamper_member_byte_trailer_left(sctx, snaphash_mode, pk):
    from snappy_amd import SnaphashError
    data = _flip_in_big(pk, pk["forms"]["stored"]["data"])
    assert len(data) == len(pk["forms"]["stored"]["data"])
    with sctx.snap_open(snap_of(pk, "stored", data=data)) as s:
        with pytest.raises(SnaphashError) as e:
            s.audit()
        assert e.value.code == EFORMAT


def test_tamper_bz2_block_crc(sctx, snaphash_mode, pk):
    from snappy_amd import SnaphashError
    d = pk["forms"]["bz2"]["data"]
    assert d[4:10] == bytes.fromhex("314159265359")
    data = d[:12] + bytes([d[12] ^ 1]) + d[13:]
    with sctx.snap_open(snap_of(pk, "bz2", data=data)) as s:
        with pytest.raises(SnaphashError) as e:
            s.audit()
        assert e.value.code == EFORMAT


def _edit(yaml, old, new):
    assert yaml.count(old) == 1, old
    return yaml.replace(old, new)


def _drop_record(yaml, name):
    lines = yaml.decode().split("\n")
    at = lines.index("- name: " + name)
    end = at + 1
    while end < len(lines) and lines[end].startswith("  "):
        end += 1
    return "\n".join(lines[:at] + lines[end:]).encode()


@pytest.mark.parametrize("form", ["pygz", "bz2"])
def test_tamper_yaml(sctx, snaphash_mode, pk, form):
    y = pk["forms"][form]["yaml"]
    first = y[16:17]
    cases = [
        (_edit(y, b"archive-sha512: " + y[16:48], b"archive-sha512: " + (b"0" if first != b"0" else b"1") + y[17:48]), (6, "archive-sha512")),
        (_drop_record(y, "bin/one"), (2, "bin/one")),
        (y + b"- name: zzz\n  mode: drwxr-xr-x\n", (1, "zzz")),
        (_edit(y, b"size: %d\n" % S.BIG, b"size: %d\n" % (S.BIG + 1)), (3, S.BIG_NAME)),
        (_edit(y, b"mode: frwxr-xr-x", b"mode: frw-r--r--"), (5, "bin/one")),
    ]
    for yaml, want in cases:
        with sctx.snap_open(snap_of(pk, form, yaml=yaml)) as s:
            assert s.audit()[0] == want, want


def test_no_hashes_yaml(sctx, snaphash_mode, pk, tmp_path):
    with sctx.snap_open(snap_of(pk, "pygz", yaml=None)) as s:
        assert s.audit()[0] == (1, "hashes.yaml")
        assert s.unpack(str(tmp_path / "a"), verify=True)[0] == (1, "hashes.yaml")
        assert s.unpack(str(tmp_path / "b"), verify=False)[0] is None
        assert os.path.exists(str(tmp_path / "b" / S.BIG_NAME))


def test_dotdot_member_is_refused(sctx, snaphash_mode, pk, tmp_path):
    from snappy_amd import SnaphashError
    data = S.gz(S.tar_files([("./ok", b"fine"), ("../evil", b"x")]))
    with sctx.snap_open(snap_of(pk, "pygz", data=data)) as s:
        with pytest.raises(SnaphashError) as e:
            s.unpack(str(tmp_path / "t"), verify=False)
        assert e.value.code == ECONTENT
        assert not os.path.exists(str(tmp_path / "evil"))


def test_container_errors(sctx, snaphash_mode, pk, tmp_path):
    from snappy_amd import SnaphashError
    p = str(tmp_path / "x.snap")
    with open(p, "wb") as f:
        f.write(S.ar_pack([("debian-binary", b"2.0\n"), ("control.tar.gz", S.control_tar_gz(b"{}\n")), ("data.tar.xz", b"\xfd7zXZ\0")]))
    with sctx.snap_open(p) as s:
        with pytest.raises(SnaphashError) as e:
            s.meta_member("package.yaml")
        assert e.value.code == EINVAL and "Can not handle data.tar.xz" in str(e.value)
        assert s.control_member("manifest") == b"{}\n"  # the other tar is still read
    with open(p, "wb") as f:
        f.write(b"!<arch>\nshort")
    with pytest.raises(SnaphashError) as e:
        sctx.snap_open(p)
    assert e.value.code == EFORMAT
    with open(p, "wb") as f:
        f.write(S.ar_pack([("debian-binary", b"2.0\n")]))
    with sctx.snap_open(p) as s:
        with pytest.raises(SnaphashError) as e:
            s.audit()
        assert e.value.code == EFORMAT and "control.tar" in str(e.value)


def test_clickdeb_mirror(sctx, snaphash_mode, pk, tmp_path):
    from snappy_amd.clickdeb import ClickDeb
    with ClickDeb.open(snap_of(pk, "bz2"), ctx=sctx) as d:
        assert d.meta_member("package.yaml") == b"name: hello\nversion: 1.0\n"
        assert d.control_member("manifest") == b"{}\n"
        assert d.audit() is None
        assert d.unpack(str(tmp_path)) is None
        assert d.stats()["data_decodes"] == 1


@pytest.mark.kernels_only("the command-line tool names its own flags")
def test_cli_snap_verbs(pk, tmp_path):
    """The shell's view: `snaphash snap audit` and `snap unpack` on a package of the builder, exit code 1 on a mismatch."""
    cli = os.path.join(ROOT, "snappy_amd", "bin", "snaphash")
    good = snap_of(pk, "pygz")
    r = subprocess.run([cli, "-g", "-s", "snap", "audit", good], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "OK\n", r.stderr
    assert "CRCs: 1 on the device" in r.stderr
    r = subprocess.run([cli, "snap", "unpack", str(tmp_path), good], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "OK\n", r.stderr
    assert os.path.getsize(str(tmp_path / S.BIG_NAME)) == S.BIG
    r = subprocess.run([cli, "snap", "cat-meta", "package.yaml", good], capture_output=True)
    assert r.returncode == 0 and r.stdout == b"name: hello\nversion: 1.0\n"
    y = pk["forms"]["pygz"]["yaml"]
    bad = snap_of(pk, "pygz", yaml=_edit(y, b"size: %d\n" % S.BIG, b"size: 1\n"))
    r = subprocess.run([cli, "snap", "audit", bad], capture_output=True, text=True)
    assert r.returncode == 1 and "size differs" in r.stderr
