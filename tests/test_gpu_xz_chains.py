""".xz with any filter chain liblzma reads -- up to three of Delta, x86, PowerPC, IA64, ARM, ARM-Thumb, SPARC in front of
LZMA2 -- written and read, in both configurations (conftest.py snaphash_mode): the producer with a chain against its host
model byte for byte and through liblzma, chain = [x86] against filter = x86, the self-check over a chain, the option
refusals; the install side with SNAPHASH_UNXZ_CHAINS over the producer's files, liblzma's own files and hand-built files whose
Blocks and Streams carry different chains (tests/xzfilt_cases.py), who undid the chains, the refusals without the flag
unchanged; a tree through tar_create_xz with a chain and back through tar_unpack_xz with Verify; a .snap built with a chain,
opened with chains=True, audited and unpacked against tarfile, and refused by a session without it; the command line."""
import ctypes
import hashlib
import io
import lzma
import os
import subprocess
import tarfile

import pytest

import trees
import xzfilt_cases as F
from conftest import ROOT
from snappy_amd import Context, _lib, clickdeb
from test_xzfilt_host import xf, encode as host_encode  # noqa: F401  (the host harness: the producer's host model)

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "snappy_amd", "bin", "snaphash")
CHAINS = F.PRODUCER_CHAINS
chain_id = lambda c: "_".join(F.NAMES[f[0] if isinstance(f, tuple) else f] for f in c)


def named(chain):
    """the chain as the Python layer takes it by name: [("delta", 2), "x86"]"""
    return [(F.NAMES[f[0]], f[1]) if isinstance(f, tuple) else F.NAMES[f] for f in chain]


def _data(n=3 * 65536 + 4321, seed=90):
    return F.mixed(n, seed)


@pytest.mark.kernels_only("the .xz producer of a buffer has no host side to plan: both configurations run the same kernels")
@pytest.mark.parametrize("chain", CHAINS, ids=chain_id)
def test_producer_is_its_host_model_and_both_decoders_read_it(snaphash_mode, xf, chain):
    data = _data()
    with Context(device=0) as c:
        for bs in (65536, 131072):
            z = c.xz_buffer(data, bs, chain=chain)
            st = c.xz_filter_stats()
            rc, model = host_encode(xf, data, bs, chain)
            assert rc == 0 and z == model, (chain, bs)
            assert lzma.decompress(z) == data
            first = chain[0][0] if isinstance(chain[0], tuple) else chain[0]
            assert st["filter"] == first and st["device_blocks"] == -(-len(data) // bs) and st["host_blocks"] == 0 and st["device_ms"] > 0, st
            assert c.xz_buffer(data, bs, chain=named(chain)) == z  # by name
            assert c.unxz_buffer(z, chains=True) == data
            on = c.xz_buffer(data, bs, chain=chain, self_check=True)  # the chunks walked, the whole chain undone and compared
            assert on == z and c.xz_selfcheck_stats()["chunks"] == -(-len(data) // 65536)
        assert c.xz_buffer(b"", 65536, chain=chain) == c.xz_buffer(b"", 65536)
        for check in (0, 1, 10):  # the Check is over the unfiltered bytes, whichever it is
            assert lzma.decompress(c.xz_buffer(data, 65536, check=check, chain=chain)) == data


@pytest.mark.kernels_only("the .xz producer of a buffer has no host side to plan: both configurations run the same kernels")
def test_chain_of_one_is_the_filter_and_the_refusals_leave_no_output(snaphash_mode):
    data = _data(2 * 65536 + 7)
    with Context(device=0) as c:
        for f in ("x86", "arm", "armthumb"):
            assert c.xz_buffer(data, 65536, chain=[f]) == c.xz_buffer(data, 65536, filter=f)
        plain = c.xz_buffer(data, 65536)
        # a 48-byte struct with chain_len 0 is the 32-byte one; so is a 40-byte one whatever lies behind it
        buf = ctypes.create_string_buffer(data, len(data))
        for size, words in ((48, []), (40, [4]), (32, [3 | 2 << 8])):
            opt = _lib.xz_options(0, 65536, 4, 0, 0, [4])
            opt.struct_size, opt.chain_len = size, len(words)
            for k, w in enumerate(words):
                opt.chain[k] = w
            p, n = ctypes.c_void_p(), ctypes.c_size_t()
            assert _lib.lib().snaphash_xz_buffer_ex(c._h, ctypes.addressof(buf), len(data), ctypes.byref(opt), ctypes.byref(p), ctypes.byref(n)) == 0
            assert ctypes.string_at(p.value, n.value) == plain, size
            _lib.lib().snaphash_free(p)
        bad = [dict(chain=[3, 4, 5, 6]), dict(chain=[2]), dict(chain=[10]), dict(chain=[0x21]), dict(chain=[("delta", 0)]), dict(chain=[("delta", 257)]),
               dict(chain=[("x86", 1)]), dict(chain=[("sparc", 4)]), dict(chain=["x86"], filter="x86"), dict(chain=[("delta", 1)], filter=4)]
        for kw in bad:
            p, n = ctypes.c_void_p(1), ctypes.c_size_t(1)
            opt = _lib.xz_options(0, 65536, 4, _lib.bcj_filter(kw.get("filter")), 0, kw["chain"])
            rc = _lib.lib().snaphash_xz_buffer_ex(c._h, ctypes.addressof(buf), len(data), ctypes.byref(opt), ctypes.byref(p), ctypes.byref(n))
            assert rc == _lib.EINVAL and p.value is None and n.value == 0, kw
        for f in (3, 5, 6, 9):  # `filter` itself keeps to its three ids
            with pytest.raises(_lib.SnaphashError) as e:
                c.xz_buffer(b"abc", 0, filter=f)
            assert e.value.code == _lib.EINVAL
        assert c.xz_buffer(data, 65536) == plain  # the ctx survives


def test_install_side_takes_every_chain_when_asked(snaphash_mode):
    files = [f for f in F.chain_files() if not f[0].startswith("chain_") or f[0].count("_") == 3][::7]  # a seventh of the three-filter chains
    files += [f for f in F.chain_files() if f[0].startswith(("mixed_blocks", "two_streams", "delta_dist", "sparc_offset_4"))]
    with Context(device=0) as c:
        for name, z, plain in files:
            if plain is None:
                continue
            assert c.unxz_buffer(z, chains=True) == plain, name
            st, us = c.xz_filter_stats(), c.unpack_stats()
            if snaphash_mode == "gpu_only":
                assert st["host_blocks"] == 0 and st["device_ms"] > 0 and us["gpu_segments"] == us["segments"], (name, st, us)
            else:
                assert st["device_blocks"] == 0, (name, st)
            if name.startswith("mixed_blocks"):  # six Blocks, one without a chain: a Block counts once, however long its chain
                assert st["device_blocks"] + st["host_blocks"] == 5 and st["filter"] == F.IA64, (name, st)
            assert c.unxz_buffer(z, chains=True, bcj=True) == plain, name  # both flags: the wider one holds
        # liblzma's own files: one Block; two Streams with different chains
        data = _data(150000, 21)
        one = F.liblzma_chain_file(data, [(F.DELTA, 3), F.X86, F.SPARC])
        two = F.liblzma_chain_file(data, [F.POWERPC]) + F.liblzma_chain_file(data[:70000], [F.IA64, (F.DELTA, 2)], lzma.CHECK_SHA256)
        assert c.unxz_buffer(one, chains=True) == data and c.unxz_buffer(two, chains=True) == data + data[:70000]
        for z, text in ((one, "xz: unsupported filter 0x03"), (two, "xz: unsupported filter 0x05")):  # without the flag: as before
            for kw in ({}, {"bcj": True}):
                with pytest.raises(_lib.SnaphashError) as e:
                    c.unxz_buffer(z, **kw)
                assert e.value.code == _lib.EINVAL and str(e.value).endswith(text), (kw, str(e.value))
        bad = _lib.UnxzOptions(ctypes.sizeof(_lib.UnxzOptions), 2)  # bit value 2 stays no flag, alone or beside the new one
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        for flags in (2, 6):
            bad.flags = flags
            assert _lib.lib().snaphash_unxz_buffer_ex(c._h, ctypes.cast(ctypes.c_char_p(one), ctypes.c_void_p), len(one), ctypes.byref(bad), ctypes.byref(p),
                                                      ctypes.byref(n)) == _lib.EINVAL


def test_refused_chains_stay_refused_with_the_flag(snaphash_mode):
    with Context(device=0) as c:
        for name, z, plain in F.chain_files():
            if plain is not None:
                continue
            with pytest.raises(_lib.SnaphashError) as e:
                c.unxz_buffer(z, chains=True)
            assert e.value.code in (_lib.EINVAL, _lib.EFORMAT), name
            if name in ("ia64_offset_8", "powerpc_offset_2", "delta_props_2_bytes"):
                assert e.value.code == _lib.EFORMAT, name
            if name == "arm64_0x0a":
                assert e.value.code == _lib.EINVAL and str(e.value).endswith("xz: unsupported filter 0x0A")
        name, z, plain = next(f for f in F.chain_files() if f[0] == "chain_delta_x86_powerpc")
        assert c.unxz_buffer(z, chains=True) == plain  # the ctx survives


def _tree(tmp_path):
    sizes = [0, 1, 4095, 65536, 65537, 300000, 12, 100000, 5]
    build, _ = trees.make_synthetic_tree(str(tmp_path), sizes)
    with open(os.path.join(build, "d0000", "code.bin"), "wb") as f:  # something every filter of the chains changes
        f.write(F.mixed(400000, 8))
    return build


def _same_tree(build, out):
    for dp, _, fns in os.walk(build):
        if os.path.basename(dp) == "DEBIAN":
            continue
        for f in fns:
            p = os.path.join(dp, f)
            assert open(os.path.join(out, os.path.relpath(p, build)), "rb").read() == open(p, "rb").read(), p


def test_tree_through_tar_create_with_a_chain_and_back(snaphash_mode, tmp_path):
    build = _tree(tmp_path)
    arc = str(tmp_path / "data.tar.xz")
    chain = [("delta", 3), "x86", "sparc"]
    with Context(device=0) as c:
        y, dig = c.tar_create_xz(arc, build, with_hashes=True, block_size=131072, chain=chain, self_check=True)
        raw = open(arc, "rb").read()
        assert dig == hashlib.sha512(raw).digest()
        fs = c.xz_filter_stats()
        tar = lzma.decompress(raw)
        assert fs["filter"] == 3 and fs["device_blocks"] == -(-len(tar) // 131072), fs
        plain_arc = str(tmp_path / "plain.tar.xz")
        y0, _ = c.tar_create_xz(plain_arc, build, with_hashes=True, block_size=131072)
        assert lzma.decompress(open(plain_arc, "rb").read()) == tar and y0 != y  # the same tar stream in another archive
        out = str(tmp_path / "tree")
        mismatch, dig2 = c.tar_unpack_xz(arc, out, y, chains=True)
        assert mismatch is None and dig2 == dig
        _same_tree(build, out)
        for kw in ({}, {"bcj": True}):
            with pytest.raises(_lib.SnaphashError) as e:
                c.tar_unpack_xz(arc, str(tmp_path / "tree2"), y, **kw)
            assert e.value.code == _lib.EINVAL
        assert clickdeb.UnpackXz(arc, str(tmp_path / "tree3"), ctx=c, chains=True) is None


def test_snap_with_a_chain_built_opened_audited_unpacked(snaphash_mode, tmp_path):
    build = _tree(tmp_path)
    os.makedirs(os.path.join(build, "DEBIAN"), exist_ok=True)
    with open(os.path.join(build, "DEBIAN", "control"), "wb") as f:
        f.write(b"Package: chains\n")
    with Context(device=0) as c:
        w = clickdeb.ClickDeb.create(str(tmp_path / "c.snap"), ctx=c).build(build, check=True, codec="xz", chain=[("delta", 2), "powerpc"], block_size=131072)
        assert c.xz_filter_stats()["filter"] == 3
        with clickdeb.ClickDeb.open(w.path, ctx=c, xz=True, chains=True) as deb:
            assert deb.members()[-1][0] == "data.tar.xz" and deb.audit() is None
            assert deb.unpack(str(tmp_path / "out")) is None
        _same_tree(build, str(tmp_path / "out"))
        with c.snap_open(w.path, xz=True, chains=True) as s:  # the member itself, against liblzma and tarfile
            name, off, size = s.members()[-1][:3]
        member = open(w.path, "rb").read()[off:off + size]
        assert hashlib.sha512(member).digest() == w.archive_digest
        names = {m.name for m in tarfile.open(fileobj=io.BytesIO(lzma.decompress(member)))}
        assert "./d0000/code.bin" in names
        with clickdeb.ClickDeb.open(w.path, ctx=c, xz=True) as deb:  # a session without chains refuses, and says which filter
            with pytest.raises(_lib.SnaphashError) as e:
                deb.audit()
            assert e.value.code == _lib.EINVAL and "xz: unsupported filter 0x03" in str(e.value)
        for flags in (_lib.SNAP_XZ_CHAINS, 2, _lib.SNAP_XZ | 2):  # the new flag needs SNAPHASH_SNAP_XZ; bit value 2 stays refused
            with pytest.raises(_lib.SnaphashError) as e:
                _lib.Snap(c, w.path, _opt=_lib.SnapOpenOptions(ctypes.sizeof(_lib.SnapOpenOptions), flags))
            assert e.value.code == _lib.EINVAL, flags


@pytest.mark.kernels_only("the command line makes its own contexts: the configuration does not enter")
def test_cli_round_trip_with_a_chain(snaphash_mode, tmp_path):
    build = _tree(tmp_path)
    arc = str(tmp_path / "data.tar.xz")
    out = subprocess.run([CLI, "-s", "build-xz", "-F", "delta:3,x86,sparc", "-B", "128", build, arc], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    raw = open(arc, "rb").read()
    assert out.stdout.split() == [hashlib.sha512(raw).hexdigest(), arc]
    assert "build-xz: filter 0x03: " in out.stderr
    tar = lzma.decompress(raw)
    ypath = os.path.join(build, "DEBIAN", "hashes.yaml")
    assert subprocess.run([CLI, "unpack-xz", "-F", arc, str(tmp_path / "no"), ypath], capture_output=True).returncode == 2  # without -A: as before
    subprocess.check_call([CLI, "unpack-xz", "-A", arc, str(tmp_path / "tree"), ypath])
    assert open(os.path.join(str(tmp_path / "tree"), "d0000", "code.bin"), "rb").read() == open(os.path.join(build, "d0000", "code.bin"), "rb").read()
    subprocess.check_call([CLI, "unxz", "-A", arc, str(tmp_path / "tar")])
    assert (tmp_path / "tar").read_bytes() == tar
    # a single old name still sets `filter`; a word that is no filter still exits 2
    one = subprocess.run([CLI, "xz", arc, str(tmp_path / "a.xz"), "-F", "x86"], capture_output=True)
    assert one.returncode == 0 and (tmp_path / "a.xz").read_bytes()[12 + 1] & 3 == 1
    for word in ("mips", "delta:257", "delta:1,x86,arm,sparc"):
        assert subprocess.run([CLI, "xz", arc, str(tmp_path / "b.xz"), "-F", word], capture_output=True).returncode == 2, word
    # the .snap: built with a chain, audited with -x -A, refused with -x alone
    with open(os.path.join(build, "DEBIAN", "control"), "wb") as f:
        f.write(b"Package: chains\n")
    snap = str(tmp_path / "c.snap")
    subprocess.check_call([CLI, "snap", "build", "-Z", "xz", "-F", "delta:2,powerpc", build, snap], stdout=subprocess.DEVNULL)
    subprocess.check_call([CLI, "snap", "-x", "-A", "audit", snap])
    assert subprocess.run([CLI, "snap", "-x", "audit", snap], capture_output=True).returncode == 2
