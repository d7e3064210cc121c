"""snaphash_snap_build with the data member in the caller's codec (snappy_amd/csrc/snapbuild.inc, snaphash_snap_build_options
.data_codec) through ClickDeb.create(path).build(dir, codec=...): data.tar.xz and data.tar.bz2 held byte for byte against the
stand-alone producers on the same ctx, against Python's lzma / bz2 / tarfile, hashlib and the oracle's hashes.yaml, and
against the install side's own audit and unpack; the producers' self-checks behind check=True; the entry as it was for
every caller that names no codec; the refusals; and one ctx building every codec in turn.  In both configurations; every
test states what it expects, so the two runs cannot differ."""
import bz2
import ctypes
import gzip
import hashlib
import io
import lzma
import os
import tarfile

import pytest

import snap_cases as S
import trees
from deflate_check_streams import payload

pytestmark = pytest.mark.gpu

EINVAL = -1
MTIME = 1445212800
SIZES = [0, 1, 111, 127, 128, 129, 1000, 4096, 65536, 65537, 100000, 3, 77, 5000, 64, 8, 16]
CHUNK = 65536
# codec, build()'s options, the same for tar_create_xz / tar_create_bz2, the suffix
CASES = {
    "xz": ("xz", {}, {}),
    "xz-opts": ("xz", dict(block_size=CHUNK, xz_check="sha256", filter="x86", level=1), dict(block_size=CHUNK, check=10, filter="x86", level=1)),
    "bz2": ("bz2", {}, {}),
    "bz2-L1": ("bz2", dict(level=1), dict(level=1)),
}


def make_tree(root, control=b"Package: hello\nVersion: 1.0\n"):
    """a synthetic tree of tests/trees.py (incompressible members), one 200 KiB text file, a symlink, and DEBIAN/ with control
    and manifest: a tar stream of several 64 KiB chunks, .xz Blocks of 64 KiB and level 1 bzip2 blocks"""
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


def member_bytes(blob, members, name):
    off, size = {m[0]: (m[1], m[2]) for m in members}[name]
    return blob[off:off + size]


def names(codec):
    return ["debian-binary", "_click-binary", "control.tar.gz", "data.tar." + codec]


def standalone(ctx, codec, path, build, opts, **kw):
    """the stand-alone producer of the codec over the tree with the DEBIAN exclude -> (yaml, digest)"""
    create = ctx.tar_create_xz if codec == "xz" else ctx.tar_create_bz2
    return create(path, build, build + "/DEBIAN", with_hashes=True, **opts, **kw)


def listing(tar_bytes):
    """(name, type, size, permission bits, link target) of every member but the root's: tarCreate writes the mode field as Go's
    FileInfoHeader does, with the file type's bits, tarfile the permission bits alone"""
    with tarfile.open(fileobj=io.BytesIO(tar_bytes)) as t:
        return [(m.name, m.type, m.size, m.mode & 0o7777, m.linkname) for m in t.getmembers() if m.name not in (".", "./")]


def no_temporaries(snap):
    d = os.path.dirname(snap)
    left = [n for n in os.listdir(d) if n.startswith(os.path.basename(snap) + ".")]
    assert not left, left


def selfcheck_units(ctx, codec):
    return ctx.xz_selfcheck_stats()["chunks"] if codec == "xz" else ctx.bz2_selfcheck_stats()["blocks"]


def expected_units(codec, opts, tar_bytes):
    """LZMA2 chunks (64 KiB of the stream each; a Block is a whole number of them) or bzip2 blocks (80 000 x level - 128 bytes
    of the stream each, the producer's piece) of a data member"""
    if codec == "xz":
        return -(-tar_bytes // CHUNK)
    return -(-tar_bytes // (80000 * opts.get("level", 9) - 128))


def build_pair(ctx, build, snap_a, kw_a, snap_b, kw_b):
    """Two builds whose DEBIAN/hashes.yaml -- rewritten by each, and carried by control.tar.gz with its mtime in whole seconds --
    has the same mtime: the pair is taken again if a second ticked between them."""
    from snappy_amd.clickdeb import ClickDeb
    yaml_path = os.path.join(build, "DEBIAN", "hashes.yaml")
    for attempt in range(4):
        a = ClickDeb.create(snap_a, ctx=ctx).build(build, mtime=MTIME, **kw_a)
        second = int(os.stat(yaml_path).st_mtime)
        b = ClickDeb.create(snap_b, ctx=ctx).build(build, mtime=MTIME, **kw_b)
        if int(os.stat(yaml_path).st_mtime) == second:
            return a, b
    pytest.fail("four pairs of builds each straddled a second")


@pytest.mark.parametrize("case", list(CASES))
def test_build_read_back_and_self_check(sctx, snaphash_mode, oracle, tmp_path, umask022, case):
    from snappy_amd.clickdeb import ClickDeb
    codec, opts, tc_opts = CASES[case]
    build = make_tree(str(tmp_path))
    snap, snap2 = str(tmp_path / "plain.snap"), str(tmp_path / "checked.snap")
    w, w2 = build_pair(sctx, build, snap, dict(codec=codec, **opts), snap2, dict(codec=codec, check=True, **opts))
    checked_units = selfcheck_units(sctx, codec)   # of the checked build, the ctx's last producer call so far
    blob = open(snap, "rb").read()
    no_temporaries(snap)
    no_temporaries(snap2)
    # the file and its digests
    assert hashlib.sha512(blob).digest() == w.snap_digest and w.build_stats["snap_bytes"] == len(blob)
    ref = str(tmp_path / ("ref.tar." + codec))
    ref_yaml, ref_digest = standalone(sctx, codec, ref, build, tc_opts)
    with ClickDeb.open(snap, ctx=sctx, xz=True) as d:
        mem = d.members()
        assert [m[0] for m in mem] == names(codec)
        assert member_bytes(blob, mem, "debian-binary") == b"2.0\n" and member_bytes(blob, mem, "_click-binary") == b"0.4\n"
        data = member_bytes(blob, mem, "data.tar." + codec)
        assert data == open(ref, "rb").read(), "the data member is not what the stand-alone producer writes for the tree"
        assert hashlib.sha512(data).digest() == w.archive_digest == ref_digest
        assert w.build_stats["data_bytes"] == len(data)
        # Python's decoder reads it, and the tar is the tree's
        tar = lzma.decompress(data) if codec == "xz" else bz2.decompress(data)
        assert w.build_stats["tar_bytes"] == len(tar) >= 4 * CHUNK
        want = [e for e in listing(S.tar_of(build)) if e[0] != "./DEBIAN" and not e[0].startswith("./DEBIAN/")]
        # (the same members: tarCreate walks in filepath.Walk's pre-order, the builder directory by directory)
        assert sorted(listing(tar)) == sorted(want) and w.build_stats["members"] >= len(want)
        if case == "xz-opts":
            assert data[7] == 10 and lzma.decompress(data, format=lzma.FORMAT_XZ) == tar   # Check SHA-256 in the Stream Flags
        if case == "bz2-L1":
            assert data[:4] == b"BZh1"
        # hashes.yaml: the oracle's for that member, in the tree and in control.tar.gz
        want_yaml = oracle.hashes_yaml(build, ref)
        assert ref_yaml == want_yaml
        assert open(os.path.join(build, "DEBIAN", "hashes.yaml"), "rb").read() == want_yaml
        assert d.control_member("hashes.yaml") == want_yaml
        ctl = gzip.decompress(member_bytes(blob, mem, "control.tar.gz"))
        with tarfile.open(fileobj=io.BytesIO(ctl)) as t:
            assert sorted(m.name for m in t.getmembers()) == ["./control", "./hashes.yaml", "./manifest"]
        # the round trip: the install side's audit and unpack
        assert d.audit() is None
        target = str(tmp_path / "out")
        os.mkdir(target)
        assert d.unpack(target, verify=True) is None
        tree = {k: v for k, v in S.tree_listing(build).items() if k != "DEBIAN" and not k.startswith("DEBIAN/")}
        assert S.tree_listing(target) == tree
    # the self-check: not a byte different, and it walked the control member's DEFLATE chunks and the data member's own units
    assert open(snap2, "rb").read() == blob
    assert w2.snap_digest == w.snap_digest and w2.archive_digest == w.archive_digest
    assert w.build_stats["check_chunks"] == 0
    units = expected_units(codec, opts, len(tar))
    assert units >= (2 if opts else 1)
    assert w2.build_stats["check_chunks"] == -(-len(ctl) // CHUNK) + units
    assert w2.build_stats["check_ms"] > 0
    assert checked_units == units
    # the producer's own flag inside the options checks the data member alone
    snap3 = str(tmp_path / "flag.snap")
    w3 = ClickDeb.create(snap3, ctx=sctx).build(build, mtime=MTIME, codec=codec, self_check=True, **opts)
    assert w3.build_stats["check_chunks"] == units and selfcheck_units(sctx, codec) == units
    assert w3.archive_digest == w.archive_digest
    if codec == "xz":
        fs = sctx.xz_filter_stats()
        assert (fs["filter"], fs["device_blocks"]) == ((4, -(-len(tar) // CHUNK)) if opts else (0, 0))
    # and a build without one says so
    ClickDeb.create(snap3, ctx=sctx).build(build, mtime=MTIME, codec=codec, **opts)
    assert selfcheck_units(sctx, codec) == 0


def raw_build(ctx, build, snap, opt):
    """snaphash_snap_build with `opt` as it is (a ctypes structure or None) -> (rc, archive digest, snap digest)"""
    from snappy_amd import _lib
    adig, sdig = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    st = _lib.SnapBuildStats()
    st.struct_size = ctypes.sizeof(_lib.SnapBuildStats)
    p = None if opt is None else ctypes.cast(ctypes.pointer(opt), ctypes.POINTER(_lib.SnapBuildOptions))
    rc = _lib.lib().snaphash_snap_build(ctx._h, os.fsencode(build), os.fsencode(snap), p, adig, sdig, ctypes.byref(st))
    return rc, adig.raw, sdig.raw


class Options16(ctypes.Structure):  # snaphash_snap_build_options as it was before it named a codec
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("mtime", ctypes.c_int64)]


def test_callers_that_name_no_codec(sctx, snaphash_mode, tmp_path, umask022):
    """opt == NULL, the 16-byte struct, and codec "gz" through the grown struct all write the file the entry always wrote: the
    data member is tarCreate's, and the files are the same byte for byte (the NULL build's mtime is "now": the others are
    given the one it wrote)."""
    from snappy_amd import _lib
    from snappy_amd.clickdeb import ClickDeb
    assert ctypes.sizeof(Options16) == 16 and ctypes.sizeof(_lib.SnapBuildOptions) == 40 and _lib.SnapBuildOptions.data_codec.offset == 16
    build = make_tree(str(tmp_path))
    yaml_path = os.path.join(build, "DEBIAN", "hashes.yaml")
    null, old, grown = (str(tmp_path / n) for n in ("null.snap", "old.snap", "grown.snap"))
    for attempt in range(4):
        rc, adig, sdig = raw_build(sctx, build, null, None)
        assert rc == 0
        second = int(os.stat(yaml_path).st_mtime)
        mtime = int(open(null, "rb").read()[8 + 16:8 + 28])
        rc2, adig2, sdig2 = raw_build(sctx, build, old, Options16(16, 0, mtime))
        assert rc2 == 0
        w = ClickDeb.create(grown, ctx=sctx).build(build, mtime=mtime, codec="gz")
        if int(os.stat(yaml_path).st_mtime) == second:
            break
    else:
        pytest.fail("four rounds of builds each straddled a second")
    blob = open(null, "rb").read()
    assert open(old, "rb").read() == blob and open(grown, "rb").read() == blob
    assert sdig == sdig2 == w.snap_digest == hashlib.sha512(blob).digest() and adig == adig2 == w.archive_digest
    ref = str(tmp_path / "ref.tar.gz")
    ref_digest = sctx.tar_create(ref, build, build + "/DEBIAN", with_hashes=True)[1]
    with ClickDeb.open(null, ctx=sctx) as d:
        mem = d.members()
        assert [m[0] for m in mem] == names("gz")
        assert member_bytes(blob, mem, "data.tar.gz") == open(ref, "rb").read() and ref_digest == adig
        assert d.audit() is None
    # the 16-byte struct with the self-check flag, as its callers set it
    rc, adig3, _ = raw_build(sctx, build, old, Options16(16, _lib.BUILD_CHECK, mtime))
    assert rc == 0 and adig3 == adig
    for n in (null, old, grown):
        no_temporaries(n)


def test_refusals(sctx, snaphash_mode, tmp_path, umask022):
    from snappy_amd import SnaphashError, _lib
    from snappy_amd.clickdeb import ClickDeb
    build = make_tree(str(tmp_path))
    snap = str(tmp_path / "refused.snap")
    size = ctypes.sizeof(_lib.SnapBuildOptions)

    def nothing_left():
        assert not os.path.exists(snap)
        no_temporaries(snap)
        assert not os.path.exists(os.path.join(build, "DEBIAN", "hashes.yaml"))   # refused before any work

    def refused(text, **kw):
        with pytest.raises(SnaphashError) as e:
            ClickDeb.create(snap, ctx=sctx).build(build, mtime=MTIME, **kw)
        assert e.value.code == EINVAL and text in str(e.value), str(e.value)
        nothing_left()

    refused("data_codec", codec=3)
    refused("not data_codec", codec="gz", filter="x86")      # xz options with codec gz
    refused("not data_codec", codec="gz", level=1)
    refused("not data_codec", codec="bz2", block_size=CHUNK)
    # the producers' own refusals, in their words
    refused("xz: the level is 0 (greedy parse) or 1 (priced parse)", codec="xz", level=2)
    refused("xz: the filter is 0 (none), 4 (x86), 7 (ARM) or 8 (ARM-Thumb)", codec="xz", filter=5)
    refused("xz: the Check is 0 (none), 1 (CRC-32), 4 (CRC-64) or 10 (SHA-256)", codec="xz", xz_check=2)
    refused("xz: the block size is a multiple of 64 KiB from 64 KiB to 4 MiB, or 0", codec="xz", block_size=1000)
    refused("bzip2: the level is 1 to 9, or 0 for 9", codec="bz2", level=10)
    # the raw struct: a reserved word that is not 0, options of the other producer, a size between the two structs
    xo = _lib.XzOptions(ctypes.sizeof(_lib.XzOptions), 0, 0, 4, 0, 0)
    bo = _lib.Bz2Options(ctypes.sizeof(_lib.Bz2Options), 0, 1)
    cases = [_lib.SnapBuildOptions(size, 0, MTIME, 2, 1), _lib.SnapBuildOptions(size, 0, MTIME, 0, 7),
             _lib.SnapBuildOptions(size, 0, MTIME, 2, 0, None, ctypes.pointer(bo)), _lib.SnapBuildOptions(size, 0, MTIME, 1, 0, ctypes.pointer(xo), None),
             _lib.SnapBuildOptions(24, 0, MTIME, 2), _lib.SnapBuildOptions(12, 0, MTIME), _lib.SnapBuildOptions(size, 4, MTIME, 2)]
    for opt in cases:
        assert raw_build(sctx, build, snap, opt)[0] == EINVAL
        nothing_left()
    # a bad options struct behind the pointer is the producer's to refuse
    bad = _lib.XzOptions(8, 0, 0, 4, 0, 0)
    assert raw_build(sctx, build, snap, _lib.SnapBuildOptions(size, 0, MTIME, 2, 0, ctypes.pointer(bad), None))[0] == EINVAL
    assert "snaphash_xz_options.struct_size" in _lib.lib().snaphash_last_error(sctx._h).decode()
    nothing_left()
    # and the ctx builds every codec afterwards
    for codec in ("xz", "bz2", "gz"):
        ClickDeb.create(snap, ctx=sctx).build(build, mtime=MTIME, codec=codec)
        with ClickDeb.open(snap, ctx=sctx, xz=True) as d:
            assert [m[0] for m in d.members()] == names(codec) and d.audit() is None


def test_codecs_in_turn(sctx, snaphash_mode, tmp_path, umask022):
    """An encoder's parameters and state are one call's own: a ctx that builds gz, xz, bz2 and gz again writes each time what
    a fresh ctx writes.  (The control member carries the mtime of the DEBIAN/hashes.yaml each build rewrites, so the files are
    held member by member: the data member's bytes, and the control tar's names and contents.)"""
    from snappy_amd import Context
    from snappy_amd.clickdeb import ClickDeb
    build = make_tree(str(tmp_path))
    turns = [("gz", {}), ("xz", dict(block_size=CHUNK, filter="x86", level=1)), ("bz2", dict(level=1)), ("gz", {})]

    def parts(snap):
        blob = open(snap, "rb").read()
        with ClickDeb.open(snap, ctx=sctx, xz=True) as d:
            mem = d.members()
            ctl = gzip.decompress(member_bytes(blob, mem, "control.tar.gz"))
            with tarfile.open(fileobj=io.BytesIO(ctl)) as t:
                control = [(m.name, m.mode, t.extractfile(m).read()) for m in t.getmembers()]
            return [m[0] for m in mem], member_bytes(blob, mem, mem[3][0]), control

    mine = []
    for k, (codec, opts) in enumerate(turns):
        snap = str(tmp_path / ("turn%d.snap" % k))
        w = ClickDeb.create(snap, ctx=sctx).build(build, mtime=MTIME, codec=codec, check=bool(k & 1), **opts)
        mine.append((parts(snap), w.archive_digest))
    assert mine[0] == mine[3]
    for k, (codec, opts) in enumerate(turns[:3]):
        snap = str(tmp_path / ("fresh%d.snap" % k))
        with Context() as fresh:
            w = ClickDeb.create(snap, ctx=fresh).build(build, mtime=MTIME, codec=codec, **opts)
        assert (parts(snap), w.archive_digest) == mine[k], codec
        assert mine[k][0][0] == names(codec)


@pytest.mark.kernels_only("one round trip through the command-line tool")
def test_cli_snap_build_with_a_codec(tmp_path, umask022):
    import subprocess
    from conftest import ROOT
    cli = os.path.join(ROOT, "snappy_amd", "bin", "snaphash")
    build = make_tree(str(tmp_path))
    for args, member in ((["-c", "-Z", "xz", "-L", "1", "-F", "x86", "-C", "sha256", "-B", "64"], "data.tar.xz"), (["-Z", "bz2", "-L", "1"], "data.tar.bz2")):
        snap = str(tmp_path / ("cli-%s.snap" % member))
        r = subprocess.run([cli, "-s", "snap", "build", *args, build, snap], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert r.stdout.split()[0] == hashlib.sha512(open(snap, "rb").read()).hexdigest()
        assert "(%s " % member in r.stderr   # the verbose line names the member it wrote
        if "-c" in args:
            assert "self-check: 0 chunks" not in r.stderr and "filter 0x04" in r.stderr
        r = subprocess.run([cli, "snap", "-x", "ls", snap], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.split()[-1] == member
        r = subprocess.run([cli, "snap", "-x", "audit", snap], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == "OK", r.stderr
    # options of a producer that is not chosen: the library's refusal, and no file
    snap = str(tmp_path / "refused.snap")
    r = subprocess.run([cli, "snap", "build", "-F", "x86", build, snap], capture_output=True, text=True)
    assert r.returncode == 2 and "not data_codec" in r.stderr and not os.path.exists(snap)
    r = subprocess.run([cli, "snap", "build", "-Z", "lzma", build, snap], capture_output=True, text=True)
    assert r.returncode == 2 and "usage:" in r.stderr


def test_done_when(sctx, snaphash_mode, tmp_path, umask022):
    from snappy_amd.clickdeb import ClickDeb
    build = make_tree(str(tmp_path))
    p = str(tmp_path / "p.snap")
    ClickDeb.create(p, ctx=sctx).build(build, codec="xz", level=1, filter="x86")
    with ClickDeb.open(p, ctx=sctx, xz=True) as d:
        assert d.audit() is None
