"""The .bz2 producer with its options and its self-check (snaphash_bzip2_buffer_ex, snaphash_tar_create_bz2_ex,
snaphash_get_bz2_selfcheck_stats), in both configurations (conftest.py snaphash_mode): the bytes with the check on are the bytes
with it off and the bytes of the entries that have no options, for every bz2enc_cases input at levels 1 and 9; the statistics
count every block written; a tree goes through tar at level 1 with the check on an engine whose staging holds one block -- the
partial byte crosses slots and both pinned buffers -- and comes back through libbz2 + tarfile and through the library's own
install side; the refusals; the command line."""
import bz2
import ctypes
import hashlib
import io
import os
import subprocess
import tarfile

import pytest

import bz2enc_cases as E
import trees
import xz_cases as X
from conftest import ROOT
from snappy_amd import Context, _lib, clickdeb

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "snappy_amd", "bin", "snaphash")


def options(flags=0, level=0):
    return _lib.Bz2Options(ctypes.sizeof(_lib.Bz2Options), flags, level)


def buffer_ex(c, data, opt, want_rc=0):
    """snaphash_bzip2_buffer_ex itself: opt a Bz2Options, or None for a null pointer."""
    p, n = ctypes.c_void_p(), ctypes.c_size_t()
    buf = ctypes.create_string_buffer(data, max(len(data), 1))
    rc = _lib.lib().snaphash_bzip2_buffer_ex(c._h, ctypes.addressof(buf), len(data), ctypes.byref(opt) if opt is not None else None, ctypes.byref(p),
                                             ctypes.byref(n))
    assert rc == want_rc, (rc, _lib.lib().snaphash_last_error(c._h))
    if rc:
        assert p.value is None
        return None
    try:
        return ctypes.string_at(p.value, n.value)
    finally:
        _lib.lib().snaphash_free(p)


def tar_ex(c, tarname, source_dir, exclude_prefix, opt, want_rc=0):
    """snaphash_tar_create_bz2_ex itself, without hashes.yaml: -> the archive digest."""
    dig, n = ctypes.create_string_buffer(64), ctypes.c_size_t()
    rc = _lib.lib().snaphash_tar_create_bz2_ex(c._h, os.fsencode(tarname), os.fsencode(source_dir), os.fsencode(exclude_prefix) if exclude_prefix else None,
                                               ctypes.byref(opt) if opt is not None else None, None, ctypes.byref(n), dig)
    assert rc == want_rc, rc
    return dig.raw


def blocks_of(n, level):
    return (n + E.piece(level) - 1) // E.piece(level)


@pytest.mark.kernels_only("the .bz2 producer of a buffer has no host side to plan: both configurations run the same kernels")
@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("level", [1, 9])
def test_same_bytes_with_the_check_on_and_off(snaphash_mode, level, half):
    with Context(device=0) as c:
        for name, data in E.cases()[half::2]:  # (every input, in two tests a level)
            want = c.bzip2_buffer(data, level)  # snaphash_bzip2_buffer
            off = buffer_ex(c, data, options(0, level))
            assert c.bz2_selfcheck_stats() == {"blocks": 0, "ms": 0.0}, name
            on = c.bzip2_buffer(data, level, self_check=True)
            st = c.bz2_selfcheck_stats()
            assert on == off == want, (name, level)
            assert st["blocks"] == blocks_of(len(data), level) == c.targz_stats()["chunks"], (name, st)
            assert st["ms"] > 0 or not data, (name, st)
        assert bz2.decompress(on) == data


def test_no_options_and_all_zero_options_are_the_plain_entry(snaphash_mode):
    data = X.text(200000, 704)
    with Context(device=0) as c:
        plain = c.bzip2_buffer(data)  # level 9
        assert plain == c.bzip2_buffer(data, 9)
        assert buffer_ex(c, data, None) == plain and buffer_ex(c, data, _lib.Bz2Options()) == plain  # a null pointer; struct_size 0 and every field zero
        assert buffer_ex(c, data, options()) == plain and buffer_ex(c, data, options(0, 9)) == plain
        assert c.bz2_selfcheck_stats()["blocks"] == 0
        assert c.bzip2_buffer(data, 0, self_check=True) == plain and c.bz2_selfcheck_stats()["blocks"] == 1


def test_several_slots_and_groups_are_all_checked(snaphash_mode):
    """Staging of three level-1 pieces: 20 pieces and a bit go through seven slots; and a slot of 288 level-1 blocks, the most a
    launch of the producer takes, is two groups of the decoder's batch of 256."""
    data = X.text(20 * E.PIECE + 5, 700)
    with Context(device=0, staging_bytes=3 * E.PIECE) as c:
        on = c.bzip2_buffer(data, 1, self_check=True)
        assert c.bz2_selfcheck_stats()["blocks"] == 21 == c.targz_stats()["chunks"]
        assert on == c.bzip2_buffer(data, 1) and bz2.decompress(on) == data
    data = (X.text(1 << 20, 705) * 22)[:288 * E.PIECE]
    with Context(device=0) as c:
        on = c.bzip2_buffer(data, 1, self_check=True)
        assert c.bz2_selfcheck_stats()["blocks"] == 288 == c.targz_stats()["chunks"]
        assert on == c.bzip2_buffer(data, 1) and bz2.decompress(on) == data


def _tree(tmp_path):
    build, _ = trees.make_synthetic_tree(str(tmp_path), [0, 1, 511, 512, 513, 4096, 65536, 65537, 100000, 300000])
    with open(os.path.join(build, "d0000", "text.txt"), "wb") as f:
        f.write(X.text(400000, 701))
    os.makedirs(os.path.join(build, "DEBIAN"))
    with open(os.path.join(build, "DEBIAN", "control"), "w") as f:
        f.write("Package: x\n")
    return build


def test_tar_create_bz2_one_block_a_slot_and_the_way_back(snaphash_mode, tmp_path):
    build = _tree(tmp_path)
    out = str(tmp_path / "data.tar.bz2")
    with Context(device=0, staging_bytes=E.PIECE) as c:  # one level-1 block a slot
        yaml, digest = c.tar_create_bz2(out, build, build + "/DEBIAN", with_hashes=True, level=1, self_check=True)
        st, zs = c.bz2_selfcheck_stats(), c.targz_stats()
        raw = open(out, "rb").read()
        assert hashlib.sha512(raw).digest() == digest and raw[:4] == b"BZh1"
        tar = bz2.decompress(raw)
        assert len(tar) > 8 * E.PIECE  # (the tree: 876 628 bytes of files; several slots, so both pinned buffers take turns)
        assert st["blocks"] == zs["chunks"] == blocks_of(len(tar), 1) and st["ms"] > 0
        tf = tarfile.open(fileobj=io.BytesIO(tar))
        regs = 0
        for m in tf.getmembers():
            assert not m.name.startswith("./DEBIAN")
            if m.isreg():
                assert tf.extractfile(m).read() == open(os.path.join(build, m.name[2:]), "rb").read(), m.name
                regs += 1
        assert regs == 10
        mis, dig2 = c.tar_unpack_bz2(out, str(tmp_path / "unpacked"), yaml)
        assert mis is None and dig2 == digest
        assert open(os.path.join(str(tmp_path / "unpacked"), "d0000", "text.txt"), "rb").read() == X.text(400000, 701)
        # the same without the check: the same file
        same = str(tmp_path / "same.tar.bz2")
        assert c.tar_create_bz2(same, build, build + "/DEBIAN", level=1)[1] == digest
        assert c.bz2_selfcheck_stats()["blocks"] == 0 and open(same, "rb").read() == raw
    with Context(device=0) as c:
        # a wider engine writes the same bytes, checked or not
        wide = str(tmp_path / "wide.tar.bz2")
        assert c.tar_create_bz2(wide, build, build + "/DEBIAN", level=1, self_check=True)[1] == digest
        # through the options with the defaults, and without options: tar_create_bz2's file (level 9)
        plain, dflt, null, lvl9 = (str(tmp_path / n) for n in ("plain.tar.bz2", "dflt.tar.bz2", "null.tar.bz2", "lvl9.tar.bz2"))
        d0 = c.tar_create_bz2(plain, build, build + "/DEBIAN")[1]
        assert tar_ex(c, dflt, build, build + "/DEBIAN", options()) == d0
        assert tar_ex(c, null, build, build + "/DEBIAN", None) == d0
        assert tar_ex(c, lvl9, build, build + "/DEBIAN", options(_lib.BZ2_SELF_CHECK, 9)) == d0
        assert c.bz2_selfcheck_stats()["blocks"] == c.targz_stats()["chunks"] > 0
        assert open(plain, "rb").read() == open(dflt, "rb").read() == open(null, "rb").read() == open(lvl9, "rb").read()
        # clickdeb.tarCreate stays the reference's: no .bz2, and the flag is the .xz producer's alone
        with pytest.raises(Exception) as e:
            clickdeb.tarCreate(str(tmp_path / "cd.tar.bz2"), build, ctx=c)
        assert "unknown compression extension" in str(e.value)
        with pytest.raises(ValueError):
            clickdeb.tarCreate(str(tmp_path / "cd.tar.gz"), build, ctx=c, self_check=True)


def test_refused_options(snaphash_mode, tmp_path):
    build = _tree(tmp_path)
    out = str(tmp_path / "data.tar.bz2")
    with Context(device=0) as c:
        for opt in ([options(f) for f in (2, 4, 0x80000000, 3)] +       # an unknown flag, alone and beside the known one
                    [options(0, 10), options(1, 10), options(1, 0xffffffff)] +  # a level above 9
                    [_lib.Bz2Options(8, 1, 9), _lib.Bz2Options(16, 1, 9), _lib.Bz2Options(0, 1, 0), _lib.Bz2Options(0, 0, 9)]):  # struct_size
            buffer_ex(c, b"abc", opt, _lib.EINVAL)
            tar_ex(c, out, build, None, opt, _lib.EINVAL)
            assert not os.path.exists(out)
        with pytest.raises(_lib.SnaphashError) as e:
            c.bzip2_buffer(b"abc", 10, self_check=True)
        assert e.value.code == _lib.EINVAL
        with pytest.raises(_lib.SnaphashError) as e:
            c.tar_create_bz2(str(tmp_path / "data.tar.gz"), build, level=1, self_check=True)
        assert e.value.code == _lib.EINVAL and "unknown compression extension" in str(e.value)
        assert bz2.decompress(c.bzip2_buffer(b"still works", 0, self_check=True)) == b"still works"  # the ctx survives
        assert c.bz2_selfcheck_stats()["blocks"] == 1


def test_cli_build_bz2_with_the_check_and_unpack(snaphash_mode, tmp_path):
    build = _tree(tmp_path)
    arc = str(tmp_path / "data.tar.bz2")
    out = subprocess.run([CLI, "-s", "build-bz2", "-c", "-L", "1", build, arc], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    raw = open(arc, "rb").read()
    assert out.stdout.split() == [hashlib.sha512(raw).hexdigest(), arc] and raw[:4] == b"BZh1"
    tar = bz2.decompress(raw)
    assert "build-bz2: self-check: %d blocks, " % blocks_of(len(tar), 1) in out.stderr
    ypath = os.path.join(build, "DEBIAN", "hashes.yaml")
    subprocess.check_call([CLI, "unpack-bz2", arc, str(tmp_path / "tree"), ypath])
    for dp, _, fs in os.walk(build):
        for f in fs:
            p = os.path.join(dp, f)
            rel = os.path.relpath(p, build)
            if not rel.startswith("DEBIAN"):
                assert open(os.path.join(str(tmp_path / "tree"), rel), "rb").read() == open(p, "rb").read(), rel
    # the plain form still is what it was, and -c alone changes no byte of it
    os.unlink(ypath)
    a, b = str(tmp_path / "a.tar.bz2"), str(tmp_path / "b.tar.bz2")
    subprocess.check_call([CLI, "build-bz2", build, a])
    os.unlink(ypath)
    subprocess.check_call([CLI, "build-bz2", "-c", build, b])
    assert open(a, "rb").read() == open(b, "rb").read() and open(a, "rb").read()[:4] == b"BZh9"
    assert subprocess.run([CLI, "build-bz2", "-x", build, a], capture_output=True).returncode == 2
    assert subprocess.run([CLI, "build-bz2", "-L", "10", build, a], capture_output=True).returncode == 2
    # bzip2 -c
    data = X.text(300000, 702) + X.rnd(70000, 703)
    (tmp_path / "in").write_bytes(data)
    out = subprocess.run([CLI, "-s", "bzip2", "-L", "1", "-c", str(tmp_path / "in"), str(tmp_path / "on.bz2")], capture_output=True, text=True)
    assert out.returncode == 0 and "bzip2: self-check: %d blocks, " % blocks_of(len(data), 1) in out.stderr, out.stderr
    subprocess.check_call([CLI, "bzip2", "-L", "1", str(tmp_path / "in"), str(tmp_path / "off.bz2")])
    assert (tmp_path / "on.bz2").read_bytes() == (tmp_path / "off.bz2").read_bytes() and bz2.decompress((tmp_path / "on.bz2").read_bytes()) == data
    out = subprocess.run([CLI, "bzip2", "-c", str(tmp_path / "in"), str(tmp_path / "on9.bz2")], capture_output=True, text=True)
    assert out.returncode == 0 and (tmp_path / "on9.bz2").read_bytes()[:4] == b"BZh9"
