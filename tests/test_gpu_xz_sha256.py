"""The .xz Check id 10 (SHA-256) on the GPU, on both sides of the library and in both configurations (conftest.py
snaphash_mode): the install side reads it -- under FLAG_GPU_ONLY sha256_ranges_kernel takes the Check of every Block the
LZMA2 kernel decoded, out of the decoded stream in HBM, and snaphash_get_xz_check_stats says who took which -- and the
producer writes it (snaphash_xz_buffer_check), with CRC-32, CRC-64 or no Check beside it.  The files the install side
reads come from tests/xz_cases.py's builders and are held against liblzma first; what the producer writes is read by
liblzma, by the install side, and held byte for byte against the host model (tests/sha256_host_harness.cpp)."""
import io
import lzma
import os
import subprocess
import tarfile

import pytest

import xz_cases as X
from conftest import ROOT
from snappy_amd import Context, _lib, getHashes
from test_gpu_unpack import tree_view
from test_sha256_host import load_sha, model_xz

pytestmark = pytest.mark.gpu

GPU_BLOCK_MAX = 4 << 20  # kXzGpuBlockMax (xz_kernels.h)
CLI = os.path.join(ROOT, "snappy_amd", "bin", "snaphash")
DEVICE_KEYS = ("device_crc32", "device_crc64", "device_sha256")


@pytest.fixture(scope="module")
def sh():
    return load_sha()


def decode(c, mode, z, plain, sha_blocks, host_checks=0, crc32_blocks=0):
    """z through unxz_buffer; the Check statistics: under gpu_only the kernels took sha_blocks SHA-256 Checks and
    crc32_blocks CRC-32 ones and host threads host_checks; planned: no kernel took any."""
    assert X.ref_decompress(z) == plain
    assert c.unxz_buffer(z) == plain
    st = c.xz_check_stats()
    if mode == "gpu_only":
        assert (st["device_sha256"], st["device_crc32"], st["device_crc64"], st["host_checks"]) == (sha_blocks, crc32_blocks, 0, host_checks), st
    else:
        assert all(st[k] == 0 for k in DEVICE_KEYS) and st["device_check_ms"] == 0, st
        assert st["host_checks"] == sha_blocks + crc32_blocks + host_checks, st
    return st


# ---- the install side ---------------------------------------------------------------------------------------------------

def test_container_cases_with_check_10(snaphash_mode):
    cases = {name: (z, plain) for name, z, plain in X.container_cases()}
    with Context(device=0) as c:
        decode(c, snaphash_mode, *cases["check_10"], sha_blocks=4)
        decode(c, snaphash_mode, *cases["streams_padding"], sha_blocks=2, crc32_blocks=2)


def test_blocks_at_every_alignment_meet_their_stored_checks(snaphash_mode):
    """Blocks of 0, 1, 55, ... bytes of output one after another: they begin at the alignments 0, 1, 8, 15 and 7 of the
    decoded stream, and the lengths are those where the tail takes one block or two."""
    sizes = [0, 1, 55, 56, 63, 64, 65, 119, 120, 4097]
    data = X.text(sum(sizes), 31)
    blocks, at = [], 0
    for n in sizes:
        blocks.append(X.raw_lzma2(data[at:at + n]))
        at += n
    starts = [sum(sizes[:k]) % 16 for k in range(len(sizes))]
    assert set(starts) == {0, 1, 8, 15, 7}
    with Context(device=0) as c:
        decode(c, snaphash_mode, X.xz_file(blocks, X.CHECK_SHA256), data, sha_blocks=len(sizes))


def test_130_blocks_more_than_two_waves(snaphash_mode):
    data = X.text(130 * 300, 32)
    blocks = [X.raw_lzma2(data[i:i + 300]) for i in range(0, len(data), 300)]
    with Context(device=0) as c:
        decode(c, snaphash_mode, X.xz_file(blocks, X.CHECK_SHA256, sizes_in_header=True), data, sha_blocks=130)


@pytest.mark.parametrize("which", [0, 3])
def test_flipped_check_field_is_eformat(snaphash_mode, which):
    data = X.text(50000, 33)
    s = X.Stream([X.raw_lzma2(data[i:i + 12500]) for i in range(0, 50000, 12500)], X.CHECK_SHA256)
    assert X.ref_decompress(s.data) == data
    with Context(device=0) as c:
        for at in (s.parts[which]["check"], s.parts[which]["end"] - 1):  # the field's first byte and its last
            bad = X._flip(s.data, at)
            assert X.refuses(X.ref_decompress, bad)
            with pytest.raises(_lib.SnaphashError) as e:
                c.unxz_buffer(bad)
            assert e.value.code == _lib.EFORMAT
            if snaphash_mode == "gpu_only":  # (a host thread's verdict on a Block is "xz: corrupt block", as before)
                assert "xz: block check mismatch" in str(e.value), str(e.value)
        assert c.unxz_buffer(s.data) == data  # the same context decodes a good file


def test_block_over_the_gpu_cap_keeps_the_host_check(snaphash_mode):
    big = bytes(GPU_BLOCK_MAX + 1)  # zeros: a long Block that costs the host decoder little
    small = X.text(100000, 34)
    s = X.Stream([X.raw_lzma2(small), X.raw_lzma2(big, dict_size=1 << 16), X.raw_lzma2(small)], X.CHECK_SHA256)
    with Context(device=0) as c:
        decode(c, snaphash_mode, s.data, small + big + small, sha_blocks=2, host_checks=1)
        bad = X._flip(s.data, s.parts[1]["check"])
        assert X.refuses(X.ref_decompress, bad)
        with pytest.raises(_lib.SnaphashError) as e:  # the host thread's Check still bites
            c.unxz_buffer(bad)
        assert e.value.code == _lib.EFORMAT


def test_unpack_xz_with_verify_of_a_check_10_package(snaphash_mode, tmp_path):
    files = {"bin/run": (b"#!/bin/sh\necho hi\n" * 40, 0o755), "share/text": (X.text(150000, 35), 0o644), "share/blob": (X.rnd(70001, 36), 0o640),
             "empty": (b"", 0o644)}
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w", format=tarfile.GNU_FORMAT) as t:
        for d in ("bin", "share"):
            ti = tarfile.TarInfo("./" + d)
            ti.type, ti.mode = tarfile.DIRTYPE, 0o755
            t.addfile(ti)
        for name, (data, mode) in sorted(files.items()):
            ti = tarfile.TarInfo("./" + name)
            ti.size, ti.mode = len(data), mode
            t.addfile(ti, io.BytesIO(data))
    raw = buf.getvalue()
    z = X.xz_file([X.raw_lzma2(raw[i:i + 50001]) for i in range(0, len(raw), 50001)], X.CHECK_SHA256)  # Blocks at odd offsets
    assert lzma.decompress(z) == raw
    arc = str(tmp_path / "data.tar.xz")
    with open(arc, "wb") as f:
        f.write(z)
    nblocks = (len(raw) + 50000) // 50001
    old = os.umask(0o022)
    try:
        with Context(device=0) as c:
            assert c.tar_unpack_xz(arc, str(tmp_path / "plain"))[0] is None
            yaml = getHashes(str(tmp_path / "plain"), arc, c)
            assert c.tar_unpack_xz(arc, str(tmp_path / "verified"), yaml)[0] is None
            st = c.xz_check_stats()
            assert st["device_sha256"] == (nblocks if snaphash_mode == "gpu_only" else 0), st
            assert st["host_checks"] == (0 if snaphash_mode == "gpu_only" else nblocks), st
        ref = str(tmp_path / "ref")
        with tarfile.open(arc, "r:xz") as t:
            for m in t.getmembers():
                p = os.path.join(ref, os.path.normpath(m.name))
                if m.isdir():
                    os.makedirs(p, exist_ok=True)
                else:
                    with open(p, "wb") as f:
                        f.write(t.extractfile(m).read())
                os.chmod(p, m.mode & ~0o022)
    finally:
        os.umask(old)
    assert tree_view(str(tmp_path / "verified")) == tree_view(ref) == tree_view(str(tmp_path / "plain"))


# ---- the producer -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def inputs():
    return {0: b"", 1: b"x", 200000: X.text(150000, 37) + X.rnd(50000, 38)}


@pytest.mark.parametrize("check", [0, 1, 4, 10])
def test_producer_with_each_check(snaphash_mode, sh, inputs, check):
    with Context(device=0) as c:
        for n, data in inputs.items():
            z = c.xz_buffer(data, 65536, check=check)
            assert lzma.decompress(z) == data, n  # (liblzma verifies every Check)
            assert c.unxz_buffer(z) == data, n
            assert z[6:8] == bytes([0, check]) and z[-4:-2] == bytes([0, check]), n
            assert z == model_xz(sh, data, 65536, check), n
            if check == 4:
                assert z == c.xz_buffer(data, 65536), n
            if check == 10 and n == 200000 and snaphash_mode == "gpu_only":
                assert c.xz_check_stats()["device_sha256"] == 4  # our own Blocks are ones the kernels read back


def test_flipped_bit_in_our_sha256_field_is_refused(snaphash_mode, inputs):
    with Context(device=0) as c:
        z = c.xz_buffer(inputs[200000], 65536, check=10)
        index_size = (int.from_bytes(z[-8:-4], "little") + 1) * 4
        last = len(z) - 12 - index_size - 1  # the last byte of the last Block's Check field
        for at in (last, last - 31):
            bad = X._flip(z, at)
            assert X.refuses(X.ref_decompress, bad)
            with pytest.raises(_lib.SnaphashError) as e:
                c.unxz_buffer(bad)
            assert e.value.code == _lib.EFORMAT


def test_other_check_ids_are_einval_and_ctx_survives(snaphash_mode, inputs):
    with Context(device=0) as c:
        for check in (2, 11):
            with pytest.raises(_lib.SnaphashError) as e:
                c.xz_buffer(inputs[200000], 65536, check=check)
            assert e.value.code == _lib.EINVAL
        assert lzma.decompress(c.xz_buffer(inputs[200000], 65536, check=10)) == inputs[200000]


def test_cli_check_option(snaphash_mode, tmp_path, inputs):
    data = inputs[200000]
    (tmp_path / "in").write_bytes(data)
    for name, check in (("sha256", 10), ("none", 0)):
        out = tmp_path / ("out_%s.xz" % name)
        subprocess.check_call([CLI, "xz", str(tmp_path / "in"), str(out), "-B", "64", "-C", name])
        z = out.read_bytes()
        assert lzma.decompress(z) == data and z[7] == check
        subprocess.check_call([CLI, "unxz", str(out), str(tmp_path / "back")])
        assert (tmp_path / "back").read_bytes() == data
    r = subprocess.run([CLI, "xz", str(tmp_path / "in"), str(tmp_path / "bogus.xz"), "-C", "bogus"], capture_output=True)
    assert r.returncode != 0 and not (tmp_path / "bogus.xz").exists()
