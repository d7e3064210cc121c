""".xz with a BCJ filter in front of LZMA2, written and read, in both configurations (conftest.py snaphash_mode): the
producer with each filter against its host model byte for byte and through liblzma, filter 0 against the plain entry, the
self-check with a filter; the install side's _ex entries over liblzma's files and over files whose Blocks carry different
chains (tests/bcj_cases.py), who undid the filters, the plain entries' refusal unchanged, a Check over the filtered bytes
refused; a tree through tar_create_xz with x86 and back through tar_unpack_xz with Verify; a filtered call followed by a
plain one on one ctx; the command line."""
import ctypes
import hashlib
import io
import lzma
import os
import subprocess
import tarfile

import pytest

import bcj_cases as B
import trees
import xz_cases as X
from conftest import ROOT
from snappy_amd import Context, _lib, clickdeb
from test_bcj_host import bh, encode as host_encode  # noqa: F401  (the host harness: the producer's host model)

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "snappy_amd", "bin", "snaphash")


def _data(filt, n=3 * 65536 + 4321, seed=90):
    return B.code(filt, n, seed + filt)


@pytest.mark.kernels_only("the .xz producer of a buffer has no host side to plan: both configurations run the same kernels")
@pytest.mark.parametrize("filt", B.FILTERS, ids=lambda f: B.NAMES[f])
def test_producer_is_its_host_model_and_liblzma_reads_it(snaphash_mode, bh, filt):
    data = _data(filt)
    with Context(device=0) as c:
        for bs in (65536, 131072):
            z = c.xz_buffer(data, bs, filter=filt)
            st = c.xz_filter_stats()
            rc, model = host_encode(bh, data, bs, filt)
            assert rc == 0 and z == model, (B.NAMES[filt], bs)
            assert lzma.decompress(z) == data
            assert st["filter"] == filt and st["device_blocks"] == -(-len(data) // bs) and st["host_blocks"] == 0 and st["device_ms"] > 0, st
            assert c.xz_buffer(data, bs, filter=B.NAMES[filt]) == z  # by name
            # filter 0 through the _ex entry: the plain entry's bytes
            opt = _lib.XzOptions(ctypes.sizeof(_lib.XzOptions), 0, bs, 4, 0)
            assert _buffer_ex(c, data, opt) == c.xz_buffer(data, bs) != z
            assert c.xz_filter_stats() == {"filter": 0, "device_blocks": 0, "host_blocks": 0, "device_ms": 0.0}
        assert c.xz_buffer(b"", 65536, filter=filt) == c.xz_buffer(b"", 65536)
        for check in (0, 1, 10):  # the Check is over the unfiltered bytes, whichever it is
            assert lzma.decompress(c.xz_buffer(data, 65536, check=check, filter=filt)) == data


def _buffer_ex(c, data, opt):
    p, n = ctypes.c_void_p(), ctypes.c_size_t()
    buf = ctypes.create_string_buffer(data, max(len(data), 1))
    rc = _lib.lib().snaphash_xz_buffer_ex(c._h, ctypes.addressof(buf), len(data), ctypes.byref(opt), ctypes.byref(p), ctypes.byref(n))
    assert rc == 0, _lib.lib().snaphash_last_error(c._h)
    try:
        return ctypes.string_at(p.value, n.value)
    finally:
        _lib.lib().snaphash_free(p)


@pytest.mark.kernels_only("the .xz producer of a buffer has no host side to plan: both configurations run the same kernels")
def test_self_check_with_a_filter_changes_no_byte(snaphash_mode):
    with Context(device=0) as c:
        for filt in B.FILTERS:
            data = _data(filt, 5 * 65536 + 99)
            off = c.xz_buffer(data, 131072, filter=filt)
            on = c.xz_buffer(data, 131072, filter=filt, self_check=True)
            assert on == off and lzma.decompress(on) == data
            assert c.xz_selfcheck_stats()["chunks"] == 6 and c.xz_filter_stats()["device_blocks"] == 3
        # a refused filter id touches nothing
        for bad in (1, 3, 5, 6, 9, 0x21):
            with pytest.raises(_lib.SnaphashError) as e:
                c.xz_buffer(b"abc", 0, filter=bad)
            assert e.value.code == _lib.EINVAL


def test_install_side_takes_the_chain_when_asked(snaphash_mode):
    with Context(device=0) as c:
        for name, z, plain in B.good_files():
            assert c.unxz_buffer(z, bcj=True) == plain, name
            st, us = c.xz_filter_stats(), c.unpack_stats()
            filtered = 1 if name.startswith("liblzma_") else 6
            assert st["device_blocks"] + st["host_blocks"] == filtered, (name, st)
            if snaphash_mode == "gpu_only":
                assert st["host_blocks"] == 0 and st["device_ms"] > 0 and us["gpu_segments"] == us["segments"], (name, st, us)
            else:
                assert st["device_blocks"] == 0, (name, st)
            # the same file without the flag: the plain entries' refusal, as before
            for call in (lambda: c.unxz_buffer(z), lambda: c.unxz_buffer(z, bcj=False)):
                with pytest.raises(_lib.SnaphashError) as e:
                    call()
                assert e.value.code == _lib.EINVAL and "xz: unsupported filter 0x0" in str(e.value), name
        for name, z, plain in X.good_cases()[:4]:  # files without filters read the same through the _ex entry
            assert c.unxz_buffer(z, bcj=True) == plain, name
            assert c.xz_filter_stats()["device_blocks"] + c.xz_filter_stats()["host_blocks"] == 0
        # a null pointer and an all-zero struct are the plain entry
        z = B.good_files()[0][1]
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        for opt in (None, ctypes.byref(_lib.UnxzOptions())):
            rc = _lib.lib().snaphash_unxz_buffer_ex(c._h, ctypes.cast(ctypes.c_char_p(z), ctypes.c_void_p), len(z), opt, ctypes.byref(p), ctypes.byref(n))
            assert rc == _lib.EINVAL and _lib.lib().snaphash_last_error(c._h) == b"xz: unsupported filter 0x04"
        bad = _lib.UnxzOptions(ctypes.sizeof(_lib.UnxzOptions), 2)
        assert _lib.lib().snaphash_unxz_buffer_ex(c._h, ctypes.cast(ctypes.c_char_p(z), ctypes.c_void_p), len(z), ctypes.byref(bad), ctypes.byref(p),
                                                  ctypes.byref(n)) == _lib.EINVAL


def test_other_chains_and_bad_properties(snaphash_mode):
    with Context(device=0) as c:
        for name, z, text in B.other_chain_files():
            for bcj in (False, True):
                with pytest.raises(_lib.SnaphashError) as e:
                    c.unxz_buffer(z, bcj=bcj)
                assert e.value.code == _lib.EINVAL and str(e.value).endswith(text), (name, bcj, str(e.value))
        for name, z in B.refused_files():
            with pytest.raises(_lib.SnaphashError) as e:
                c.unxz_buffer(z, bcj=True)
            assert e.value.code == _lib.EFORMAT, name
            with pytest.raises(_lib.SnaphashError) as e:
                c.unxz_buffer(z)
            assert e.value.code == _lib.EINVAL, name
        with pytest.raises(_lib.SnaphashError) as e:  # a Check taken over the filtered bytes
            c.unxz_buffer(B.check_over_filtered_file(), bcj=True)
        assert e.value.code == _lib.EFORMAT
        z, plain = B.good_files()[0][1:]
        assert c.unxz_buffer(z, bcj=True) == plain  # the ctx survives


def test_a_block_larger_than_the_kernel_takes(snaphash_mode):
    """kXzGpuBlockMax is 4 MiB: a larger Block goes to a host thread in either configuration, its filter with it; the
    Blocks beside it stay where the configuration puts them."""
    unit = B.x86_code(65536, 3)
    big = unit * 65 + unit[:777]  # 4 MiB + 64 KiB + 777: compresses to a few hundred KiB
    small = B.code(B.ARM, 70000, 4)
    z = B.xz_chained([(small, [(B.ARM, b"")]), (big, [(B.X86, b"")])])
    assert len(z) < 2 << 20
    with Context(device=0) as c:
        assert c.unxz_buffer(z, bcj=True) == small + big
        st = c.xz_filter_stats()
        assert (st["device_blocks"], st["host_blocks"]) == ((1, 1) if snaphash_mode == "gpu_only" else (0, 2)), st


def _tree(tmp_path):
    sizes = [0, 1, 4095, 65536, 65537, 300000, 12, 100000, 5]
    build, _ = trees.make_synthetic_tree(str(tmp_path), sizes)
    # something the x86 filter changes: a file of calls
    with open(os.path.join(build, "d0000", "code.bin"), "wb") as f:
        f.write(B.x86_code(400000, 8))
    return build


def test_tree_through_tar_create_with_x86_and_back(snaphash_mode, tmp_path):
    build = _tree(tmp_path)
    arc = str(tmp_path / "data.tar.xz")
    with Context(device=0) as c:
        y, dig = c.tar_create_xz(arc, build, with_hashes=True, block_size=131072, filter="x86", self_check=True)
        raw = open(arc, "rb").read()
        assert dig == hashlib.sha512(raw).digest()
        fs = c.xz_filter_stats()
        tar = lzma.decompress(raw)
        assert fs["filter"] == 4 and fs["device_blocks"] == -(-len(tar) // 131072), fs
        names = {m.name for m in tarfile.open(fileobj=io.BytesIO(tar))}
        assert "./d0000/code.bin" in names
        plain_arc = str(tmp_path / "plain.tar.xz")
        y0, _ = c.tar_create_xz(plain_arc, build, with_hashes=True, block_size=131072)
        assert lzma.decompress(open(plain_arc, "rb").read()) == tar and y0 != y  # the same tar stream in another archive
        out = str(tmp_path / "tree")
        mismatch, dig2 = c.tar_unpack_xz(arc, out, y, bcj=True)
        assert mismatch is None and dig2 == dig
        for dp, _, fns in os.walk(build):
            for f in fns:
                p = os.path.join(dp, f)
                assert open(os.path.join(out, os.path.relpath(p, build)), "rb").read() == open(p, "rb").read(), p
        with pytest.raises(_lib.SnaphashError) as e:
            c.tar_unpack_xz(arc, str(tmp_path / "tree2"), y)
        assert e.value.code == _lib.EINVAL
        # clickdeb's names
        d3 = clickdeb.tarCreate(str(tmp_path / "c.tar.xz"), build, ctx=c, filter="x86")
        assert d3 == hashlib.sha512(open(str(tmp_path / "c.tar.xz"), "rb").read()).digest()
        assert clickdeb.UnpackXz(str(tmp_path / "c.tar.xz"), str(tmp_path / "tree3"), ctx=c, bcj=True) is None


@pytest.mark.kernels_only("the .xz producer of a buffer has no host side to plan: both configurations run the same kernels")
def test_a_plain_call_after_a_filtered_one(snaphash_mode):
    data = _data(B.X86, 4 * 65536 + 5)
    with Context(device=0) as fresh:
        want = fresh.xz_buffer(data, 65536)
    with Context(device=0) as c:
        f = c.xz_buffer(data, 65536, filter="x86", self_check=True)
        assert c.xz_buffer(data, 65536) == want != f
        assert c.xz_buffer(data, 65536, self_check=True) == want
        assert c.xz_buffer(data, 65536, filter="arm") not in (want, f)
        assert c.xz_buffer(data, 65536, filter="x86") == f


def test_cli_build_xz_with_a_filter_and_unpack(snaphash_mode, tmp_path):
    build = _tree(tmp_path)
    arc = str(tmp_path / "data.tar.xz")
    out = subprocess.run([CLI, "-s", "build-xz", "-F", "x86", "-B", "128", build, arc], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    raw = open(arc, "rb").read()
    assert out.stdout.split() == [hashlib.sha512(raw).hexdigest(), arc]
    assert "build-xz: filter 0x04: " in out.stderr
    tar = lzma.decompress(raw)
    ypath = os.path.join(build, "DEBIAN", "hashes.yaml")
    assert subprocess.run([CLI, "unpack-xz", arc, str(tmp_path / "no"), ypath], capture_output=True).returncode == 2  # without -F: as before
    subprocess.check_call([CLI, "unpack-xz", "-F", arc, str(tmp_path / "tree"), ypath])
    assert open(os.path.join(str(tmp_path / "tree"), "d0000", "code.bin"), "rb").read() == open(os.path.join(build, "d0000", "code.bin"), "rb").read()
    subprocess.check_call([CLI, "unxz", "-F", arc, str(tmp_path / "tar")])
    assert (tmp_path / "tar").read_bytes() == tar
    assert subprocess.run([CLI, "unxz", arc, str(tmp_path / "tar2")], capture_output=True).returncode == 2
    assert subprocess.run([CLI, "build-xz", "-F", "mips", build, arc], capture_output=True).returncode == 2
    (tmp_path / "in").write_bytes(B.code(B.THUMB, 200000, 1))
    out = subprocess.run([CLI, "-s", "xz", str(tmp_path / "in"), str(tmp_path / "t.xz"), "-F", "armthumb", "-c"], capture_output=True, text=True)
    assert out.returncode == 0 and "xz: filter 0x08: 1 blocks on the GPU" in out.stderr, out.stderr
    assert lzma.decompress((tmp_path / "t.xz").read_bytes()) == (tmp_path / "in").read_bytes()
