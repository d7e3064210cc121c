"""Block mode on the GPU (SNAPHASH_FLAG_SPLIT_BLOCKS): plain gzip streams -- zlib's and Python's, no flush points -- cut
at their DEFLATE block boundaries by the block scan kernel and decoded side by side, in both configurations
(conftest.py snaphash_mode: the inflate kernel under GPU-only, host threads by default).  Every Context here ORs the flag
into Context.DEFAULT_FLAGS.  The serial checks of the same code are in tests/test_inflate_blocks_host.py."""
import gzip
import io
import os
import tarfile
import zlib

import numpy as np
import pytest

from snappy_amd import Context, _lib, getHashes

from test_inflate_blocks_host import load_blocks, scan

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SHARE = 0.02  # host_bytes may be at most this share of a plain text stream's output


def corpus(kind, n, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
    words = [bytes(rng.integers(97, 123, size=int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(2000)]
    base = b" ".join(words[int(i)] for i in rng.integers(0, 2000, size=200000))
    return (base * (n // len(base) + 1))[:n]


def split_ctx(**kw):
    return Context(device=0, flags=Context.DEFAULT_FLAGS | _lib.FLAG_SPLIT_BLOCKS, **kw)


@pytest.fixture(scope="module")
def bh():
    return load_blocks()


def test_plain_streams_decode_in_parallel(snaphash_mode):
    text = corpus("text", 16 << 20, seed=5)
    mix = corpus("text", 5 << 20, seed=5) + corpus("random", 1 << 20, seed=6)
    with split_ctx() as c:
        for data in (text, mix):
            gz = gzip.compress(data, 9)
            assert c.gunzip_buffer(gz) == data
            st, bs = c.unpack_stats(), c.block_scan_stats()
            assert st["host_bytes"] <= HOST_SHARE * len(data), (st, bs)
            assert st["segments"] >= len(data) // (320 << 10), (st, bs)  # (a segment fits a slot: 320 Ki symbols)
            assert bs["linked"] >= 20 and bs["host_blocks"] == 0, (st, bs)
            if snaphash_mode == "gpu_only":
                assert st["gpu_segments"] == st["segments"], st
        assert c.block_scan_stats()["scan_ms"] > 0
        # Go's and dpkg's level: 6, and level 1
        for lvl in (1, 6):
            assert c.gunzip_buffer(gzip.compress(text[: 8 << 20], lvl)) == text[: 8 << 20]
            assert c.unpack_stats()["host_bytes"] <= HOST_SHARE * (8 << 20)


def test_scan_parity_with_the_cpu_checker(snaphash_mode, bh):
    """One piece: the kernel's candidates (block_scan_stats) are what inf_dynamic_ok finds on the same bytes.  A member's
    first piece is 1 MiB; a member that ends inside it, followed by a small one, is scanned exactly once."""
    tail = corpus("text", 700000, seed=10)
    with split_ctx() as c:
        for data in (corpus("text", 2400 << 10, seed=7), corpus("text", 1300 << 10, seed=8) + corpus("random", 300 << 10, seed=9)):
            gz = gzip.compress(data, 9) + gzip.compress(tail, 9)
            assert len(gzip.compress(data, 9)) - 10 < (1 << 20) <= len(gz) - 10, len(gz)
            assert c.gunzip_buffer(gz) == data + tail
            bs = c.block_scan_stats()
            piece = gz[10:10 + (1 << 20)]  # (gzip.compress writes a 10-byte header: no name)
            assert bs["bits_scanned"] == 8 * len(piece), bs
            want = scan(bh, piece)
            assert bs["candidates"] == len(want), (bs, len(want))
            assert bs["linked"] + bs["unreached"] == bs["candidates"]


def test_many_small_members_scan_a_bounded_piece_each(snaphash_mode):
    """A member's length is unknown until it is decoded: each member in block mode scans at most 1 MiB before its end,
    not the rest of the stream."""
    parts = [corpus("text", 80000, seed=40 + k) for k in range(100)]
    gz = b"".join(gzip.compress(p, 9) for p in parts)
    with split_ctx() as c:
        assert c.gunzip_buffer(gz) == b"".join(parts)
        bs = c.block_scan_stats()
        assert 0 < bs["bits_scanned"] <= 100 * 8 * (1 << 20), (len(gz), bs)


def test_flag_off_keeps_the_serial_route(snaphash_mode):
    text = corpus("text", 5 << 20, seed=5)
    plain = gzip.compress(text, 9)
    with Context(device=0) as c:
        assert c.gunzip_buffer(plain) == text
        st = c.unpack_stats()
        assert st["host_bytes"] == len(text) and st["gpu_segments"] == 0, st
        assert all(v == 0 for v in c.block_scan_stats().values())
        off = {k: v for k, v in st.items() if not k.endswith("_ms")}
    with split_ctx() as c:  # a member below the threshold stays serial under the flag too
        small = corpus("text", 1 << 20, seed=3)
        assert c.gunzip_buffer(gzip.compress(small, 9)) == small
        st = c.unpack_stats()
        assert st["host_bytes"] == len(small) and c.block_scan_stats()["bits_scanned"] == 0
        assert c.gunzip_buffer(plain) == text
        on = c.unpack_stats()
        assert on["host_bytes"] < off["host_bytes"] and on["tar_bytes"] == off["tar_bytes"]


def test_flush_streams_and_concatenated_members(snaphash_mode):
    data = corpus("text", 6 << 20, seed=11)
    with split_ctx() as c:
        prod = c.gzip_buffer(data)  # the producer's flush points, now also block candidates
        assert c.gunzip_buffer(prod) == data
        two = gzip.compress(data[:3 << 20], 9) + prod + gzip.compress(b"", 9) + gzip.compress(data[:100000], 9)
        assert c.gunzip_buffer(two) == data[:3 << 20] + data + data[:100000]


def test_small_staging_chains_cross_pieces(snaphash_mode):
    data = corpus("text", 10 << 20, seed=12) + corpus("random", 1 << 20, seed=13)
    gz = gzip.compress(data, 9)
    with split_ctx(staging_bytes=1 << 20) as c:
        assert c.gunzip_buffer(gz) == data
        st, bs = c.unpack_stats(), c.block_scan_stats()
        assert bs["bits_scanned"] >= 8 * (len(gz) - 10) and bs["host_blocks"] == 0, (st, bs)
        assert st["host_bytes"] == 0, st


def test_corrupt_plain_stream_is_eformat_and_ctx_survives(snaphash_mode):
    data = corpus("text", 4 << 20, seed=14)
    gz = bytearray(gzip.compress(data, 9))
    with split_ctx() as c:
        bad = bytes(gz[:-8]) + bytes([gz[-8] ^ 1]) + bytes(gz[-7:])  # CRC-32
        for b in (bad, bytes(gz[: len(gz) // 2]), bytes(gz[:-40])):
            with pytest.raises(_lib.SnaphashError) as e:
                c.gunzip_buffer(b)
            assert e.value.code == _lib.EFORMAT
        mid = bytearray(gz)
        for k in range(300, len(mid) - 100, len(mid) // 9):
            mid[k] ^= 0x5a
        try:
            assert c.gunzip_buffer(bytes(mid)) != data
        except _lib.SnaphashError as err:
            assert err.code == _lib.EFORMAT
        assert c.gunzip_buffer(bytes(gz)) == data


def make_build(root):
    build = os.path.join(root, "build")
    os.makedirs(os.path.join(build, "bin"))
    os.makedirs(os.path.join(build, "share", "doc"))
    files = {"bin/run": (b"#!/bin/sh\necho hi\n" * 50, 0o755), "share/big.txt": (corpus("text", 6 << 20, 21), 0o644),
             "share/blob": (corpus("random", 300000, 22), 0o640), "share/doc/README": (corpus("text", 900000, 23), 0o644),
             "empty": (b"", 0o644), "share/zeros": (bytes(50000), 0o600)}
    for name, (data, mode) in files.items():
        p = os.path.join(build, name)
        with open(p, "wb") as f:
            f.write(data)
        os.chmod(p, mode)
    os.symlink("run", os.path.join(build, "bin", "alias"))
    return build


def tree(root):
    out = {}
    for dp, dns, fns in os.walk(root):
        for n in dns + fns:
            p = os.path.join(dp, n)
            rel = os.path.relpath(p, root)
            out[rel] = os.readlink(p) if os.path.islink(p) else (open(p, "rb").read() if os.path.isfile(p) else None)
    return out


def test_tar_unpack_of_a_tarfile_archive(snaphash_mode, tmp_path):
    old = os.umask(0o022)
    try:
        build = make_build(str(tmp_path))
        arc = str(tmp_path / "data.tar.gz")
        with tarfile.open(arc, "w:gz") as t:  # zlib -9, no flush points
            t.add(build, arcname=".")
        with Context(device=0) as plain:
            assert plain.tar_unpack(arc, str(tmp_path / "serial"))[0] is None
            yaml = getHashes(str(tmp_path / "serial"), arc, plain)
        with split_ctx() as c:
            mis, dig = c.tar_unpack(arc, str(tmp_path / "nohash"))
            assert mis is None and len(dig) == 64
            assert tree(str(tmp_path / "nohash")) == tree(build)
            st = c.unpack_stats()
            assert st["host_bytes"] <= 0.05 * st["tar_bytes"] and c.block_scan_stats()["linked"] >= 20, (st, c.block_scan_stats())
            mis, _ = c.tar_unpack(arc, str(tmp_path / "verified"), yaml)
            assert mis is None
            assert tree(str(tmp_path / "verified")) == tree(build)
            # a changed member: the same mismatch snaphash_verify reports on the unpacked tree
            lines = yaml.split(b"\n")
            i = lines.index(b"- name: share/doc/README")
            k = next(j for j in range(i, len(lines)) if lines[j].startswith(b"  sha512: "))
            lines[k] = lines[k][:-1] + (b"0" if lines[k][-1:] != b"0" else b"1")
            bad = b"\n".join(lines)
            mis, _ = c.tar_unpack(arc, str(tmp_path / "tampered"), bad)
            assert mis is not None and mis == c.verify(str(tmp_path / "tampered"), bad, arc), mis
    finally:
        os.umask(old)


def test_engine_info_counts_the_block_scratch(snaphash_mode):
    data = corpus("text", 8 << 20, seed=31)
    gz = gzip.compress(data, 9)
    with split_ctx() as c:
        before = c.engine_info(0)
        assert c.gunzip_buffer(gz) == data
        after = c.engine_info(0)
        if snaphash_mode == "gpu_only":  # the block slots live in HBM
            assert after["hbm_bytes"] - before["hbm_bytes"] >= 64 << 20, (before, after)
        else:  # the piece and the scans' candidates, in HBM and pinned memory
            assert after["hbm_bytes"] > before["hbm_bytes"] and after["pinned_bytes"] > before["pinned_bytes"], (before, after)
