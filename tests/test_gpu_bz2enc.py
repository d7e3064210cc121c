"""Writing data.tar.bz2 on the GPU: snaphash_bzip2_buffer (the RLE1, BWT, MTF, coding and concatenation kernels of
bzip2_enc_kernels.hip and the bzip2 CRC kernels), snaphash_bwt_device and snaphash_tar_create_bz2, in both configurations
(conftest.py snaphash_mode), over the inputs of tests/bz2enc_cases.py.  libbz2's verdict (Python's bz2) carries the tests;
the bytes are also held against the host model of the same header (tests/bz2enc_host_harness.cpp) -- a self-comparison
that shows no lane, workgroup, slot or launch leaks into the output -- and the library's own install side reads the files
back."""
import bz2
import hashlib
import io
import os
import re
import subprocess
import tarfile

import numpy as np
import pytest

import bz2enc_cases as B
import snap_cases as S
import trees
import xz_cases as X
from conftest import ROOT
from snappy_amd import Context, _lib
from test_bz2enc_host import all_cases, bwt, encode, load_model

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "snappy_amd", "bin", "snaphash")
P1 = B.PIECE


@pytest.fixture(scope="module")
def be():
    return load_model()


@pytest.fixture(scope="module")
def model(be):
    """(name, level) -> (data, the host model's file), computed once and left alone; level 1 first, so that a ctx going
    through them allocates for each level once."""
    out = {}
    for name, data, lv in sorted(all_cases(be), key=lambda c: c[2]):
        out[(name, lv)] = (data, encode(be, data, lv)[0])
    return out


def test_bzip2_buffer_on_every_input(snaphash_mode, model):
    with Context(device=0) as c:
        for (name, lv), (data, want) in model.items():
            z = c.bzip2_buffer(data, lv)
            assert z == want, (name, lv)
            assert bz2.decompress(z) == data, (name, lv)
            st = c.targz_stats()
            Pn = B.piece(lv)
            assert st["tar_bytes"] == len(data) and st["gz_bytes"] == len(z) and st["chunks"] == (len(data) + Pn - 1) // Pn, (name, lv, st)
            assert st["stored_chunks"] == 0, (name, lv)
        data, want = model[("text_%d" % (2 * P1 + 1), 9)]
        assert c.bzip2_buffer(data) == want  # level 0 is level 9


def test_refused_levels_and_a_ctx_that_survives(snaphash_mode, model):
    data, want = model[("text_%d" % (P1 + 1), 1)]
    with Context(device=0) as c:
        for bad in (10, 1 << 31):
            with pytest.raises(_lib.SnaphashError) as e:
                c.bzip2_buffer(data, bad)
            assert e.value.code == _lib.EINVAL, bad
        assert c.bzip2_buffer(data, 1) == want
        empty = c.bzip2_buffer(b"", 1)
        assert empty == model[("text_0", 1)][1] and len(empty) == 14 and bz2.decompress(empty) == b""


def test_the_bytes_do_not_depend_on_slots_or_launches(snaphash_mode, model):
    """Six pieces at level 1 in one call, and again by engines whose staging holds one, two and three pieces -- the bit
    carried from slot to slot and the concatenation are in every one -- and after another input went through the ctx."""
    data, want = model[("six_pieces", 1)]
    with Context(device=0) as c:
        assert c.bzip2_buffer(data, 1) == want and c.targz_stats()["chunks"] == 6
        assert c.bzip2_buffer(X.rnd(100000, 71), 1) != want
        assert c.bzip2_buffer(data, 1) == want
    for pieces in (1, 2, 3):
        with Context(device=0, staging_bytes=pieces * P1) as c:
            assert c.bzip2_buffer(data, 1) == want, pieces
            assert c.targz_stats()["chunks"] == 6
    with Context(device=0, staging_bytes=65536) as c:  # a block's input must fit the engine's staging
        with pytest.raises(_lib.SnaphashError) as e:
            c.bzip2_buffer(data, 1)
        assert e.value.code == _lib.EINVAL


def naive_bwt(b, width=None):
    """Sorted cyclic rotations, equal ones by start index: (last column, origPtr).  width: compare that many bytes only
    (exact when they tell all rotations apart, which is checked)."""
    n = len(b)
    w = width or n
    d = b * (w // n + 2)
    keys = [(d[i:i + w], i) for i in range(n)]
    keys.sort()
    if width:
        assert all(keys[j][0] != keys[j + 1][0] for j in range(n - 1))
    return bytes(b[i - 1] for _, i in keys), [i for _, i in keys].index(0)


def test_bwt_device(snaphash_mode, be):
    import torch
    import random
    r = random.Random(9)
    ranges = [bytes(r.randrange(4) for _ in range(n)) for n in (1, 2, 63, 64, 65, 1023, 1024, 1025)]
    ranges += [b"abc" * 400, b"q" * 777, X.rnd(100000, 91)]
    want = [naive_bwt(d, 32 if len(d) == 100000 else None) for d in ranges]
    assert want[-1] == bwt(be, ranges[-1])  # (the host model on the way)
    with Context(device=0) as c:
        for order in (list(range(len(ranges))), list(reversed(range(len(ranges))))):
            buf, offs = bytearray(b"\x5a" * 7), []
            for k in order:
                offs.append(len(buf))
                buf += ranges[k] + b"\x5a" * (1 + k % 5)
            lens = [len(ranges[k]) for k in order]
            d_in = torch.tensor(np.frombuffer(bytes(buf), dtype=np.uint8)).cuda()
            d_last = torch.full((len(buf),), 0xA5, dtype=torch.uint8, device="cuda")
            d_op = torch.full((len(order) + 2,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
            c.bwt_device(d_in.data_ptr(), np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint64), d_last.data_ptr(),
                         d_op.data_ptr() + 4)
            torch.cuda.synchronize()
            last, ops = bytes(d_last.cpu().numpy()), d_op.cpu().numpy()
            assert bytes(d_in.cpu().numpy()) == bytes(buf)  # the input is what it was
            assert ops[0] == ops[-1] == 0x7FFFFFFF
            expect = bytearray(b"\xa5" * len(buf))
            for j, k in enumerate(order):
                expect[offs[j]:offs[j] + lens[j]] = want[k][0]
                assert ops[1 + j] == want[k][1], (k, len(ranges[k]))
            assert last == bytes(expect)
        for bad in (0, 900001):
            with pytest.raises(_lib.SnaphashError) as e:
                c.bwt_device(d_in.data_ptr(), np.array([0], dtype=np.uint64), np.array([bad], dtype=np.uint64), d_last.data_ptr(), d_op.data_ptr())
            assert e.value.code == _lib.EINVAL


def _tree(tmp_path):
    build, _ = trees.make_simple_tree(str(tmp_path / "t"))
    with open(os.path.join(build, "big.bin"), "wb") as f:
        f.write(X.text(1600000, 80) + X.rnd(70001, 81))  # three blocks at level 9
    return build


def test_tar_create_bz2(snaphash_mode, tmp_path, be):
    build = _tree(tmp_path)
    out, out_gz = str(tmp_path / "data.tar.bz2"), str(tmp_path / "data.tar.gz")
    with Context(device=0) as c:
        for with_hashes in (False, True):
            yaml, digest = c.tar_create_bz2(out, build, build + "/DEBIAN", with_hashes)
            st = c.targz_stats()
            raw = open(out, "rb").read()
            assert hashlib.sha512(raw).digest() == digest and st["gz_bytes"] == len(raw) and st["stored_chunks"] == 0
            tar = bz2.decompress(raw)
            assert st["tar_bytes"] == len(tar) and len(tar) % 512 == 0 and st["chunks"] == (len(tar) + B.piece(9) - 1) // B.piece(9) == 3
            assert raw == encode(be, tar, 9)[0]  # the host model's bytes
            tf = tarfile.open(fileobj=io.BytesIO(raw), mode="r:bz2")
            names = tf.getnames()
            assert "./bin/bar" in names and "./big.bin" in names and not any("DEBIAN" in n for n in names)
            for m in tf.getmembers():
                assert (m.uid, m.gid, m.uname, m.gname) == (0, 0, "root", "root")
                if m.isreg():
                    assert tf.extractfile(m).read() == open(os.path.join(build, m.name[2:]), "rb").read(), m.name
            if with_hashes:
                yaml_gz, _ = c.tar_create(out_gz, build, build + "/DEBIAN", True)
                strip = lambda y: re.sub(rb"archive-sha512: [0-9a-f]+\n", b"", y)
                assert b"archive-sha512: " + hashlib.sha512(raw).hexdigest().encode() + b"\n" in yaml
                assert strip(yaml) == strip(yaml_gz) and strip(yaml) != yaml
                # the install side: the file with its yaml, and a .snap put together around it
                target = str(tmp_path / "unpacked")
                os.mkdir(target)
                assert c.tar_unpack_bz2(out, target, yaml)[0] is None
                assert open(os.path.join(target, "big.bin"), "rb").read() == open(os.path.join(build, "big.bin"), "rb").read()
                snap = str(tmp_path / "p.snap")
                with open(snap, "wb") as f:
                    f.write(S.ar_pack([("debian-binary", b"2.0\n"), ("control.tar.gz", S.control_tar_gz(yaml)), ("data.tar.bz2", raw)]))
                with c.snap_open(snap) as s:
                    assert s.audit()[0] is None
                    target2 = str(tmp_path / "unpacked2")
                    os.mkdir(target2)
                    assert s.unpack(target2, verify=True)[0] is None
                    assert s.stats()["data_decodes"] == 1
                assert S.tree_listing(target2) == S.tree_listing(target)
    # an engine whose staging holds one block: three slots, the partial byte carried from one pinned output buffer to the
    # other and back, with and without the fused hashes -- the same file
    with Context(device=0, staging_bytes=B.piece(9)) as c:
        for with_hashes in (False, True):
            out1 = str(tmp_path / ("one%d.tar.bz2" % with_hashes))
            yaml1, digest1 = c.tar_create_bz2(out1, build, build + "/DEBIAN", with_hashes)
            assert open(out1, "rb").read() == raw and digest1 == digest and c.targz_stats()["chunks"] == 3
            assert yaml1 == (yaml if with_hashes else None)
    with Context(device=0) as c:
        for name in ("data.tar.gz", "data.tar.xz", "data.bz2x", "bz2"):
            with pytest.raises(_lib.SnaphashError) as e:
                c.tar_create_bz2(str(tmp_path / name), build, build + "/DEBIAN")
            assert e.value.code == _lib.EINVAL and "unknown compression extension" in str(e.value), name
        for entry in (c.tar_create, c.tar_create_xz):  # tarCreate's own answer to a .bz2 name stays
            with pytest.raises(_lib.SnaphashError) as e:
                entry(out, build, build + "/DEBIAN")
            assert e.value.code == _lib.EINVAL and "unknown compression extension" in str(e.value)


def test_cli_bzip2_and_build_bz2(snaphash_mode, tmp_path, model):
    data, want9 = model[("text_%d" % (2 * P1 + 1), 9)]
    _, want1 = model[("text_%d" % (2 * P1 + 1), 1)]
    src = tmp_path / "in.bin"
    src.write_bytes(data)
    flags = ["-g"] if snaphash_mode == "gpu_only" else []
    subprocess.check_call([CLI] + flags + ["bzip2", str(src), str(tmp_path / "o9.bz2")])
    subprocess.check_call([CLI] + flags + ["bzip2", "-L", "1", str(src), str(tmp_path / "o1.bz2")])
    assert (tmp_path / "o9.bz2").read_bytes() == want9 and (tmp_path / "o1.bz2").read_bytes() == want1
    for bad in (["bzip2", "-L", "10", str(src), str(tmp_path / "x.bz2")], ["bzip2", "-L", "x", str(src), str(tmp_path / "x.bz2")]):
        assert subprocess.run([CLI] + bad, capture_output=True).returncode == 2
    build = _tree(tmp_path)
    out = str(tmp_path / "cli.tar.bz2")
    line = subprocess.check_output([CLI] + flags + ["build-bz2", build, out], text=True)
    raw = open(out, "rb").read()
    assert line.split()[0] == hashlib.sha512(raw).hexdigest()
    os.remove(os.path.join(build, "DEBIAN", "hashes.yaml"))
    with Context(device=0) as c:
        c.tar_create_bz2(str(tmp_path / "api.tar.bz2"), build, build + "/DEBIAN", True)
    assert open(str(tmp_path / "api.tar.bz2"), "rb").read() == raw
    usage = subprocess.run([CLI], capture_output=True, text=True)
    assert usage.returncode == 2 and "bzip2 [-L LEVEL] IN OUT.bz2" in usage.stderr and "build-bz2 DIR OUT.tar.bz2" in usage.stderr
