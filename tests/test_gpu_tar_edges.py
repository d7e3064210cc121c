"""The tar reader behind the device entry points: the hand-made streams of tests/tar_cases.py, wrapped in gzip, bzip2
and xz, through snaphash_tar_unpack(_bz2/_xz) and the .snap session, in both configurations; and Verify out of HBM on a
tar whose regular members sit at offsets that are only 512-aligned, one per SHA-512 padding class.

ORDER MATTERS.  tar_read's member table goes to the SHA-512 kernels as a job table, and they read the decoded stream in
HBM with no check of their own.  These tests run only after tests/test_tar_host.py is green on the CPU: no archive that
tar_read accepts with an extent outside the stream may ever reach a device entry point.  Every bad case used here is
imported from tar_cases.py and asserted to carry a refusal code before it is sent anywhere; what the refusal is, and that
every entry's extent stays inside the stream, is the CPU suite's to show."""
import bz2
import gzip
import hashlib
import io
import lzma
import os
import tarfile

import pytest

import snap_cases as S
import tar_cases as T
from test_gpu_unpack import tree_view

pytestmark = pytest.mark.gpu

EIO, EFORMAT = -3, -9
CODECS = {"gz": (lambda b: gzip.compress(b, 6, mtime=0), "tar_unpack"), "bz2": (lambda b: bz2.compress(b, 1), "tar_unpack_bz2"),
          "xz": (lambda b: lzma.compress(b, format=lzma.FORMAT_XZ), "tar_unpack_xz")}
UNPACKABLE = [(n, tar) for n, tar, _ in T.good_cases() if T.unpackable(n)]


@pytest.fixture(scope="module")
def umask_022():
    old = os.umask(0o022)  # the cases' modes are what a 022 umask leaves alone: open(2) and tarfile's chmod then agree
    yield
    os.umask(old)


@pytest.fixture(scope="module")
def _ctxs():
    made = {}
    yield made
    for c in made.values():
        c.close()


@pytest.fixture
def sctx(snaphash_mode, built_lib, _ctxs):
    """A context in the configuration of this run, one per mode."""
    from snappy_amd import Context
    if snaphash_mode not in _ctxs:
        _ctxs[snaphash_mode] = Context()
    return _ctxs[snaphash_mode]


@pytest.fixture(scope="module")
def reference_trees(tmp_path_factory, umask_022):
    """What tarfile's extraction makes of every unpackable good case, once."""
    root = tmp_path_factory.mktemp("ref")
    out = {}
    for name, tar in UNPACKABLE:
        d = str(root / name)
        os.makedirs(d)
        S.extract_reference(tar, d)
        out[name] = tree_view(d)
    return out


def test_the_cases_chosen():
    assert len(UNPACKABLE) >= 28 and all(len(tar) < (1 << 20) for _, tar in UNPACKABLE)


@pytest.mark.parametrize("codec", sorted(CODECS))
def test_good_archives_unpack_as_tarfile_extracts_them(sctx, snaphash_mode, codec, reference_trees, tmp_path):
    wrap, entry = CODECS[codec]
    for name, tar in UNPACKABLE:
        arc = tmp_path / (name + ".tar." + codec)
        data = wrap(tar)
        arc.write_bytes(data)
        got = tmp_path / ("got_" + name)
        mis, dig = getattr(sctx, entry)(str(arc), str(got))
        assert mis is None, name
        assert dig == hashlib.sha512(data).digest(), name
        assert tree_view(str(got)) == reference_trees[name], name


def test_symlink_over_an_existing_file_fails_as_os_symlink_does(sctx, snaphash_mode, tmp_path):
    """The one good stream that is no unpackable tree: UnpackTar's os.Symlink answers EEXIST where a regular member of the
    name was written before, and so does symlink() here (tarfile would unlink first)."""
    from snappy_amd import SnaphashError
    tar = dict((n, t) for n, t, _ in T.good_cases())["regular_then_symlink_then_dir"]
    arc = tmp_path / "rs.tar.gz"
    arc.write_bytes(S.gz(tar))
    with pytest.raises(SnaphashError) as e:
        sctx.tar_unpack(str(arc), str(tmp_path / "t"))
    assert e.value.code == EIO
    assert open(str(tmp_path / "t" / "rs"), "rb").read() == b"r"


# ---- Verify out of HBM at hand-made offsets ------------------------------------------------------------------------------

SIZES = (0, 1, 111, 112, 127, 128, 129, 239, 240, 255, 256, 257, 65537)  # the SHA-512 padding classes, and more than one chunk
PAX_NAME = "pax/" + "p" * 130       # longer than ustar's 100 with no "/" to split at: PAX_FORMAT writes a path record
GNU_NAME = "gnu/" + "g" * 130
DUP_FIRST, DUP_SECOND = b"the first copy, not on disk" * 9, b"the second copy" * 31
OVERRIDDEN = b"o" * 777


def content(n):
    return hashlib.shake_128(b"%d" % n).digest(n)


def tarfile_blocks(fmt, entries):
    """The header and data blocks tarfile writes for these members, without the end-of-archive blocks.
    entries: (name, bytes) regular, (name, None) directory, (name, str) symlink."""
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w", format=fmt) as t:
        for name, data in entries:
            ti = tarfile.TarInfo(name)
            ti.uname = ti.gname = "root"
            if data is None:
                ti.type, ti.mode = tarfile.DIRTYPE, 0o755
                t.addfile(ti)
            elif isinstance(data, str):
                ti.type, ti.linkname, ti.mode = tarfile.SYMTYPE, data, 0o777
                t.addfile(ti)
            else:
                ti.size, ti.mode = len(data), 0o755 if len(data) & 1 else 0o644
                t.addfile(ti, io.BytesIO(data))
        end = t.offset
    return buf.getvalue()[:end]


def verify_tar(first=DUP_FIRST):
    sized = [("sized", None)] + [("sized/f%05d" % n, content(n)) for n in SIZES]
    blocks = tarfile_blocks(tarfile.USTAR_FORMAT, sized + [("dup", first), ("link", "sized/f00001")])
    blocks += tarfile_blocks(tarfile.PAX_FORMAT, [(PAX_NAME, b"named by a PAX record")])
    blocks += tarfile_blocks(tarfile.GNU_FORMAT, [(GNU_NAME, b"named by a GNU long name")])
    blocks += tarfile_blocks(tarfile.USTAR_FORMAT, [("dup", DUP_SECOND)])
    # a PAX size record over a header whose own size field is wrong (by hand: tarfile writes none for a small member)
    blocks += T.pax(T.record(b"size", b"%d" % len(OVERRIDDEN))) + T.member(b"overridden", OVERRIDDEN, size=3)
    return blocks + T.END


@pytest.fixture(scope="module")
def vt(tmp_path_factory, oracle, umask_022):
    """The tar, its gzip, tarfile's extraction and the oracle's hashes.yaml over that tree and archive."""
    tmp = tmp_path_factory.mktemp("vt")
    tar = verify_tar()
    assert len(tar) < (1 << 20)
    with tarfile.open(fileobj=io.BytesIO(tar)) as t:
        ms = {m.name: m for m in t.getmembers()}
        assert PAX_NAME in ms and GNU_NAME in ms and ms["overridden"].size == len(OVERRIDDEN)
        regular = [m for m in t.getmembers() if m.isreg()]
        assert all(m.offset_data % 512 == 0 for m in regular) and any(m.offset_data % 1024 for m in regular)
    arc = tmp / "data.tar.gz"
    arc.write_bytes(S.gz(tar))
    ref = tmp / "ref"
    ref.mkdir()
    S.extract_reference(tar, str(ref))
    yaml = oracle.hashes_yaml(str(ref), str(arc))
    # the oracle is this project's own restatement: its digests are held against hashlib here
    want = {("sized/f%05d" % n): content(n) for n in SIZES}
    want.update({"dup": DUP_SECOND, PAX_NAME: b"named by a PAX record", GNU_NAME: b"named by a GNU long name", "overridden": OVERRIDDEN})
    lines = yaml.split(b"\n")
    for name, data in want.items():
        i = lines.index(b"- name: " + name.encode())
        rec = lines[i + 1:i + 4]
        assert b"  size: %d" % len(data) in rec and b"  sha512: " + hashlib.sha512(data).hexdigest().encode() in rec, name
    assert b"archive-sha512: " + hashlib.sha512(arc.read_bytes()).hexdigest().encode() in lines
    return {"tar": tar, "arc": str(arc), "yaml": yaml, "lines": lines, "ref": tree_view(str(ref)), "tmp": tmp}


def edit_record(lines, name, field, fn):
    out = list(lines)
    i = out.index(b"- name: " + name.encode())
    for k in range(i + 1, i + 4):
        if out[k].startswith(b"  " + field + b": "):
            out[k] = fn(out[k])
            return b"\n".join(out)
    raise AssertionError("no %r in the record of %s" % (field, name))


def flip_last_hex(ln):
    return ln[:-1] + (b"0" if ln[-1:] != b"0" else b"1")


def test_verify_out_of_hbm_accepts_the_tar(sctx, snaphash_mode, vt, tmp_path):
    mis, dig = sctx.tar_unpack(vt["arc"], str(tmp_path / "ok"), vt["yaml"])
    assert mis is None
    assert dig == hashlib.sha512(open(vt["arc"], "rb").read()).digest()
    assert tree_view(str(tmp_path / "ok")) == vt["ref"]
    assert sctx.verify(str(tmp_path / "ok"), vt["yaml"], vt["arc"]) is None


def test_verify_out_of_hbm_tampers(sctx, snaphash_mode, vt, tmp_path):
    first_hex = hashlib.sha512(DUP_FIRST).hexdigest().encode()
    tampers = {
        # the record of the name present twice: the SECOND copy is on disk, so a wrong digest there must be found ...
        "second_duplicate_digest": (edit_record(vt["lines"], "dup", b"sha512", flip_last_hex), (4, "dup")),
        # ... and the first copy's own digest in its place is wrong too
        "first_duplicates_digest_in_the_record": (edit_record(vt["lines"], "dup", b"sha512", lambda ln: b"  sha512: " + first_hex), (4, "dup")),
        "overridden_size": (edit_record(vt["lines"], "overridden", b"size", lambda ln: b"  size: 3"), (3, "overridden")),
        "sized_digest": (edit_record(vt["lines"], "sized/f00239", b"sha512", flip_last_hex), (4, "sized/f00239")),
        "pax_named_digest": (edit_record(vt["lines"], PAX_NAME, b"sha512", flip_last_hex), (4, PAX_NAME)),
        "gnu_named_digest": (edit_record(vt["lines"], GNU_NAME, b"sha512", flip_last_hex), (4, GNU_NAME)),
    }
    for what, (y, by_hand) in tampers.items():
        d = str(tmp_path / what)
        mis, _ = sctx.tar_unpack(vt["arc"], d, y)
        want = sctx.verify(d, y, vt["arc"])
        assert mis is not None and mis == want, (what, mis, want)
        assert mis == by_hand, what


def test_first_duplicates_content_is_not_on_disk(sctx, snaphash_mode, vt, tmp_path):
    """The bytes of the FIRST copy of the name changed in the stream (and the archive digest of the yaml with them): the
    first copy is not what an unpack leaves, so nothing mismatches -- in the pass out of HBM as in Verify on the tree."""
    changed = bytes(b ^ 0x55 for b in DUP_FIRST)
    tar = verify_tar(changed)
    assert len(tar) == len(vt["tar"]) and tar != vt["tar"]
    arc = tmp_path / "data.tar.gz"
    arc.write_bytes(S.gz(tar))
    lines = [b"archive-sha512: " + hashlib.sha512(arc.read_bytes()).hexdigest().encode() if ln.startswith(b"archive-sha512: ") else ln
             for ln in vt["lines"]]
    y = b"\n".join(lines)
    mis, _ = sctx.tar_unpack(str(arc), str(tmp_path / "t"), y)
    assert mis is None and sctx.verify(str(tmp_path / "t"), y, str(arc)) is None
    assert open(str(tmp_path / "t" / "dup"), "rb").read() == DUP_SECOND


# ---- refusals ------------------------------------------------------------------------------------------------------------

REFUSED = ("pax_size_2^64-1", "pax_size_-1", "b256_size_2^63")
A_YAML = b"archive-sha512: " + b"0" * 128 + b"\nfiles:\n- name: victim\n  size: 0\n  sha512: " + b"0" * 128 + b"\n  mode: frw-r--r--\n"


@pytest.mark.parametrize("which", REFUSED)
def test_hostile_sizes_are_eformat_everywhere(sctx, snaphash_mode, which, reference_trees, tmp_path):
    from snappy_amd import SnaphashError
    bad = {n: (tar, code) for n, tar, code in T.bad_cases()}
    tar, code = bad[which]
    assert code == T.EFORMAT == EFORMAT  # a refusal, shown on the CPU first (module docstring)
    arc = tmp_path / "bad.tar.gz"
    arc.write_bytes(S.gz(tar))
    target = tmp_path / "target"
    for yaml in (None, A_YAML):
        with pytest.raises(SnaphashError) as e:
            sctx.tar_unpack(str(arc), str(target), yaml)
        assert e.value.code == EFORMAT, (which, yaml is not None)
    snap = str(tmp_path / "bad.snap")
    S.write_snap(snap, "data.tar.gz", S.gz(tar), A_YAML)
    with sctx.snap_open(snap) as s:
        with pytest.raises(SnaphashError) as e:
            s.audit()
        assert e.value.code == EFORMAT
        with pytest.raises(SnaphashError) as e:
            s.unpack(str(target), verify=True)
        assert e.value.code == EFORMAT
    assert not target.exists()
    # the context survives: a good archive unpacks, with Verify, on the same one
    name, good = UNPACKABLE[0]
    ok = tmp_path / "ok.tar.gz"
    ok.write_bytes(S.gz(good))
    assert sctx.tar_unpack(str(ok), str(tmp_path / "ok"))[0] is None
    assert tree_view(str(tmp_path / "ok")) == reference_trees[name]
