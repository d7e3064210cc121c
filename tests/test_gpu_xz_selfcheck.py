"""The .xz producer with its options and its self-check (snaphash_xz_buffer_ex, snaphash_tar_create_xz_ex,
snaphash_get_xz_selfcheck_stats), in both configurations (conftest.py snaphash_mode): the bytes with the check on are the
bytes with it off and the bytes of the entries that have no options, for every xzenc_cases input and all four Checks; the
statistics count every chunk of every Block; a tree goes through tar, 128 KiB Blocks, SHA-256 and the check and comes back
through liblzma + tarfile and through the library's own install side; the refusals; the command line."""
import ctypes
import hashlib
import io
import lzma
import os
import subprocess
import tarfile

import pytest

import trees
import xz_cases as X
import xzenc_cases as E
from conftest import ROOT
from snappy_amd import Context, _lib, clickdeb

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "snappy_amd", "bin", "snaphash")
CHECKS = (0, 1, 4, 10)


def options(flags=0, block_size=0, check=4):
    return _lib.XzOptions(ctypes.sizeof(_lib.XzOptions), flags, block_size, check, 0)


def buffer_ex(c, data, opt):
    """snaphash_xz_buffer_ex itself: opt an XzOptions, or None for a null pointer."""
    p, n = ctypes.c_void_p(), ctypes.c_size_t()
    buf = ctypes.create_string_buffer(data, max(len(data), 1))
    rc = _lib.lib().snaphash_xz_buffer_ex(c._h, ctypes.addressof(buf), len(data), ctypes.byref(opt) if opt is not None else None, ctypes.byref(p),
                                          ctypes.byref(n))
    assert rc == 0, _lib.lib().snaphash_last_error(c._h)
    try:
        return ctypes.string_at(p.value, n.value)
    finally:
        _lib.lib().snaphash_free(p)


def tar_ex(c, tarname, source_dir, exclude_prefix, opt):
    """snaphash_tar_create_xz_ex itself, without hashes.yaml: -> the archive digest."""
    dig, n = ctypes.create_string_buffer(64), ctypes.c_size_t()
    rc = _lib.lib().snaphash_tar_create_xz_ex(c._h, os.fsencode(tarname), os.fsencode(source_dir), os.fsencode(exclude_prefix),
                                              ctypes.byref(opt) if opt is not None else None, None, ctypes.byref(n), dig)
    assert rc == 0, rc
    return dig.raw


def chunks_of(n, bs):
    bs = bs or 1 << 20
    return sum((min(bs, n - o) + E.CHUNK - 1) // E.CHUNK for o in range(0, n, bs))


@pytest.mark.kernels_only("the .xz producer of a buffer has no host side to plan: both configurations run the same kernels")
@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("check", CHECKS)
def test_same_bytes_with_the_check_on_and_off(snaphash_mode, check, half):
    with Context(device=0) as c:
        for name, data, bs in E.cases()[half::2]:  # (every input, in two tests of a few seconds each)
            want = c.xz_buffer(data, bs, check=check)  # snaphash_xz_buffer_check
            off = buffer_ex(c, data, options(0, bs, check))
            assert c.xz_selfcheck_stats() == {"chunks": 0, "ms": 0.0}, name
            on = c.xz_buffer(data, bs, check=check, self_check=True)
            st = c.xz_selfcheck_stats()
            assert on == off == want, (name, check)
            assert st["chunks"] == chunks_of(len(data), bs) == c.targz_stats()["chunks"], (name, st)
            assert st["ms"] > 0 or not data, (name, st)
        assert lzma.decompress(on) == data


def test_no_options_and_all_zero_options_are_the_plain_entry(snaphash_mode):
    data = X.text(200000, 704)
    with Context(device=0) as c:
        plain = c.xz_buffer(data)
        assert buffer_ex(c, data, None) == plain and buffer_ex(c, data, _lib.XzOptions()) == plain  # a null pointer; struct_size 0 and every field zero
        assert buffer_ex(c, data, options()) == plain
        assert c.xz_selfcheck_stats()["chunks"] == 0


def test_several_slots_and_launches_are_all_walked(snaphash_mode):
    """2 MiB of staging: a slot is two Blocks of 1 MiB, so 5 MiB + 1 go through three slots."""
    data = X.text((5 << 20) + 1, 700)
    with Context(device=0, staging_bytes=2 << 20) as c:
        on = c.xz_buffer(data, 0, self_check=True)
        st = c.xz_selfcheck_stats()
        assert st["chunks"] == chunks_of(len(data), 0) == 81
        assert on == c.xz_buffer(data, 0) and lzma.decompress(on) == data


def _tree(tmp_path):
    build, _ = trees.make_synthetic_tree(str(tmp_path), [0, 1, 511, 512, 513, 4096, 65536, 65537, 100000, 300000])
    with open(os.path.join(build, "d0000", "text.txt"), "wb") as f:
        f.write(X.text(400000, 701))
    os.makedirs(os.path.join(build, "DEBIAN"))
    with open(os.path.join(build, "DEBIAN", "control"), "w") as f:
        f.write("Package: x\n")
    return build


def test_tar_create_xz_with_options_and_the_way_back(snaphash_mode, tmp_path):
    build = _tree(tmp_path)
    out = str(tmp_path / "data.tar.xz")
    with Context(device=0) as c:
        yaml, digest = c.tar_create_xz(out, build, build + "/DEBIAN", with_hashes=True, block_size=128 << 10, check=10, self_check=True)
        st, zs = c.xz_selfcheck_stats(), c.targz_stats()
        raw = open(out, "rb").read()
        assert hashlib.sha512(raw).digest() == digest
        assert raw[6:8] == b"\x00\x0a"  # the Stream flags: SHA-256
        tar = lzma.decompress(raw)
        assert st["chunks"] == zs["chunks"] == chunks_of(len(tar), 128 << 10) and st["ms"] > 0
        tf = tarfile.open(fileobj=io.BytesIO(tar))
        regs = 0
        for m in tf.getmembers():
            assert not m.name.startswith("./DEBIAN")
            if m.isreg():
                assert tf.extractfile(m).read() == open(os.path.join(build, m.name[2:]), "rb").read(), m.name
                regs += 1
        assert regs == 10
        mis, dig2 = c.tar_unpack_xz(out, str(tmp_path / "unpacked"), yaml)
        assert mis is None and dig2 == digest
        assert open(os.path.join(str(tmp_path / "unpacked"), "d0000", "text.txt"), "rb").read() == X.text(400000, 701)
        assert c.tree(build, out) == yaml
        # tar_create's records of the same tree: everything but the archive's own digest agrees, and both carry one
        gz = str(tmp_path / "data.tar.gz")
        gyaml, gdig = c.tar_create(gz, build, build + "/DEBIAN", with_hashes=True)
        strip = lambda y: [ln for ln in y.split(b"\n") if not ln.startswith(b"archive-sha512:")]
        assert strip(yaml) == strip(gyaml) and len(strip(yaml)) == len(yaml.split(b"\n")) - 1
        assert digest.hex().encode() in yaml and gdig.hex().encode() in gyaml
        # the same without the check, and through the options with the defaults: tar_create_xz's file
        same = str(tmp_path / "same.tar.xz")
        assert c.tar_create_xz(same, build, build + "/DEBIAN", block_size=128 << 10, check=10)[1] == digest
        assert c.xz_selfcheck_stats()["chunks"] == 0 and open(same, "rb").read() == raw
        plain, dflt, null = (str(tmp_path / n) for n in ("plain.tar.xz", "dflt.tar.xz", "null.tar.xz"))
        d0 = c.tar_create_xz(plain, build, build + "/DEBIAN")[1]
        assert tar_ex(c, dflt, build, build + "/DEBIAN", options()) == d0
        assert tar_ex(c, null, build, build + "/DEBIAN", None) == d0
        assert open(plain, "rb").read() == open(dflt, "rb").read() == open(null, "rb").read()
        # clickdeb.tarCreate passes the flag through for .xz names
        cd = str(tmp_path / "cd.tar.xz")
        assert clickdeb.tarCreate(cd, build, ctx=c, self_check=True) == hashlib.sha512(open(cd, "rb").read()).digest()
        assert c.xz_selfcheck_stats()["chunks"] == c.targz_stats()["chunks"] > 0
        with pytest.raises(ValueError):
            clickdeb.tarCreate(str(tmp_path / "cd.tar.gz"), build, ctx=c, self_check=True)


def test_refused_options(snaphash_mode, tmp_path):
    build = _tree(tmp_path)
    out = str(tmp_path / "data.tar.xz")
    with Context(device=0) as c:
        def refused(fn):
            with pytest.raises(_lib.SnaphashError) as e:
                fn()
            assert e.value.code == _lib.EINVAL
        for bs in (1, 65536 + 512, 8 << 20):
            refused(lambda: c.xz_buffer(b"x" * 100, bs, self_check=True))
            refused(lambda: c.tar_create_xz(out, build, block_size=bs))
        for check in (2, 5, 11, 15, 16):
            refused(lambda: c.xz_buffer(b"x" * 100, 0, check=check, self_check=True))
            refused(lambda: c.tar_create_xz(out, build, check=check))
        assert not os.path.exists(out)
        for flags in (2, 4, 0x80000000, 3):  # an unknown flag, alone and beside the known one
            opt = _lib.XzOptions(ctypes.sizeof(_lib.XzOptions), flags, 0, 4, 0)
            p, n = ctypes.c_void_p(), ctypes.c_size_t()
            buf = ctypes.create_string_buffer(b"abc", 3)
            assert _lib.lib().snaphash_xz_buffer_ex(c._h, ctypes.addressof(buf), 3, ctypes.byref(opt), ctypes.byref(p), ctypes.byref(n)) == _lib.EINVAL
            assert p.value is None
            y, yl = ctypes.c_void_p(), ctypes.c_size_t()
            assert _lib.lib().snaphash_tar_create_xz_ex(c._h, os.fsencode(out), os.fsencode(build), None, ctypes.byref(opt), None, ctypes.byref(yl),
                                                        None) == _lib.EINVAL
        opt = _lib.XzOptions(8, 1, 0, 4, 0)  # a struct_size that is neither zero nor the struct's
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        buf = ctypes.create_string_buffer(b"abc", 3)
        assert _lib.lib().snaphash_xz_buffer_ex(c._h, ctypes.addressof(buf), 3, ctypes.byref(opt), ctypes.byref(p), ctypes.byref(n)) == _lib.EINVAL
        assert not os.path.exists(out)
        assert lzma.decompress(c.xz_buffer(b"still works", 0, self_check=True)) == b"still works"  # the ctx survives


def test_cli_build_xz_with_the_check_and_unpack(snaphash_mode, tmp_path):
    build = _tree(tmp_path)
    arc = str(tmp_path / "data.tar.xz")
    out = subprocess.run([CLI, "-s", "build-xz", "-c", "-B", "128", "-C", "sha256", build, arc], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    raw = open(arc, "rb").read()
    assert out.stdout.split() == [hashlib.sha512(raw).hexdigest(), arc]
    tar = lzma.decompress(raw)
    assert "build-xz: self-check: %d chunks, " % chunks_of(len(tar), 128 << 10) in out.stderr
    assert raw[6:8] == b"\x00\x0a"
    ypath = os.path.join(build, "DEBIAN", "hashes.yaml")
    subprocess.check_call([CLI, "unpack-xz", arc, str(tmp_path / "tree"), ypath])
    for dp, _, fs in os.walk(build):
        for f in fs:
            p = os.path.join(dp, f)
            rel = os.path.relpath(p, build)
            if not rel.startswith("DEBIAN"):
                assert open(os.path.join(str(tmp_path / "tree"), rel), "rb").read() == open(p, "rb").read(), rel
    # the plain form still is what it was, and -c alone changes no byte of it
    os.unlink(ypath)
    a, b = str(tmp_path / "a.tar.xz"), str(tmp_path / "b.tar.xz")
    subprocess.check_call([CLI, "build-xz", build, a])
    os.unlink(ypath)
    subprocess.check_call([CLI, "build-xz", "-c", build, b])
    assert open(a, "rb").read() == open(b, "rb").read()
    assert subprocess.run([CLI, "build-xz", "-x", build, a], capture_output=True).returncode == 2
    assert subprocess.run([CLI, "build-xz", "-C", "md5", build, a], capture_output=True).returncode == 2
    # xz -c
    data = X.text(300000, 702) + X.rnd(70000, 703)
    (tmp_path / "in").write_bytes(data)
    out = subprocess.run([CLI, "-s", "xz", str(tmp_path / "in"), str(tmp_path / "on.xz"), "-B", "128", "-c"], capture_output=True, text=True)
    assert out.returncode == 0 and "xz: self-check: %d chunks, " % chunks_of(len(data), 128 << 10) in out.stderr, out.stderr
    subprocess.check_call([CLI, "xz", str(tmp_path / "in"), str(tmp_path / "off.xz"), "-B", "128"])
    assert (tmp_path / "on.xz").read_bytes() == (tmp_path / "off.xz").read_bytes() and lzma.decompress((tmp_path / "on.xz").read_bytes()) == data
