"""The GPU bzip2 kernels (bzip2_kernels.hip) at the edges that are their own: the sample arithmetic of the inverse BWT
(stride, the samples, origPtr's extra sample), the shape of the permutation it walks (blocks that are exactly periodic
after RLE1: u^k has k cycles), and the RLE1 chunk boundaries (each chunk's entry state).  Every stream is compared
with bz2.decompress (libbz2).  Two test-side models make each test assert the shape it claims to cover: libbz2's RLE1
(the block's symbol count n) and the origPtr field of a block header.  The CPU suite runs the kernels' inverse BWT
helpers serially (tests/test_bzip2_host.py)."""
import bz2
import gzip
import io
import os
import random
import tarfile

import numpy as np
import pytest

from snappy_amd import Context, _lib
from test_bzip2_host import SAMPLE_NS, periodic_streams, periodic_unit, run_free, text
from test_gpu_bunzip2 import _yaml_for, check_stats, umask_022  # noqa: F401  (umask_022: a fixture)
from test_gpu_unpack import make_tree, tree_view

pytestmark = pytest.mark.gpu


def rle1_len(run):
    """Bytes libbz2's RLE1 makes of a run of `run` equal bytes: 4 + a count for 4..255, longer runs in 255s."""
    return run // 255 * 5 + (run % 255 if run % 255 < 4 else 5)


def rle1(data):
    """libbz2's RLE1 of `data` (one block's worth): a run of 4..255 equal bytes becomes the 4 bytes and a count byte
    (run - 4); a longer run is cut into runs of 255 and what is left."""
    a = np.frombuffer(data, np.uint8)
    if len(a) == 0:
        return b""
    starts = np.flatnonzero(np.concatenate(([True], a[1:] != a[:-1])))
    lens = np.diff(np.append(starts, len(a)))
    out, pos = bytearray(), 0
    for i in np.flatnonzero(lens >= 4):
        st, run = int(starts[i]), int(lens[i])
        out += data[pos:st]
        v = data[st:st + 1]
        while run >= 4:
            c = min(run, 255)
            out += v * 4 + bytes([c - 4])
            run -= c
        out += v * run
        pos = st + int(lens[i])
    out += data[pos:]
    return bytes(out)


def orig_ptr(z, block_bit=32):
    """origPtr of the block whose magic starts at block_bit (the first block of a stream: bit 32): the 24 bits after
    the 48-bit magic, the 32-bit CRC and the randomised bit."""
    bit = block_bit + 81
    v = int.from_bytes(z[bit // 8: bit // 8 + 5], "big")
    return (v >> (40 - 24 - bit % 8)) & 0xffffff


def stride_of(n):
    """The inverse BWT kernel's sample stride: 2048 walkers over n positions."""
    return -(-n // 2048)


def chunk_of(n):
    """The RLE1 kernels' chunk size: at most 1024 chunks a block, at least 64 bytes each."""
    return max(64, -(-n // 1024))


def chunk_entries(pre):
    """(chunk size, [(entry state, first byte) of every chunk after the first]) of a block's RLE1 form: the state is
    bz_rle1_step's run (0 fresh, 1-3 equal bytes so far, 4: the chunk's first byte is a count)."""
    cs = chunk_of(len(pre))
    run, last, out = 0, -1, []
    for i, v in enumerate(pre):
        if i and i % cs == 0:
            out.append((run, v))
        if run == 4:
            run = 0
        elif run and v == last:
            run += 1
        else:
            run, last = 1, v
    return cs, out


def decode_one_block(c, mode, data, z):
    assert bz2.decompress(z) == data
    assert c.bunzip2_buffer(z) == data, len(data)
    st = check_stats(c, mode, data, z)
    assert st["segments"] == 1, (len(data), st)


def test_periodic_blocks(snaphash_mode):
    """Blocks that are u^k after RLE1, k >= 2: the inverse BWT's permutation is k cycles, and the n-step walk from
    origPtr goes round one of them k times (the kernel once refused every such block as corrupt)."""
    classes = set()
    with Context(device=0) as c:
        for data, lv in periodic_streams():
            pre = rle1(data)
            n = len(pre)
            p = next(p for p in range(1, 1001) if n % p == 0 and pre == pre[:p] * (n // p))
            assert n // p >= 2 and n <= lv * 100000 - 19, (len(data), n, p)
            z = bz2.compress(data, lv)
            op = orig_ptr(z)
            assert op < n
            if stride_of(n) > 1:
                classes.add(op % stride_of(n) == 0)
            decode_one_block(c, snaphash_mode, data, z)
    assert classes == {True, False}, "origPtr is a multiple of the sample stride in every block, or in none"


def test_sample_arithmetic(snaphash_mode):
    """Run-free blocks at the n where the sample stride and the count of samples change (n = 2048 k + {-1, 0, 1}, the
    largest blocks of levels 1 and 9)."""
    with Context(device=0) as c:
        for n in SAMPLE_NS:
            data = run_free(n, 100 + n)
            assert len(rle1(data)) == n
            for lv in ((1, 9) if n == 99981 else (9,)):
                z = bz2.compress(data, lv)
                assert orig_ptr(z) < n
                decode_one_block(c, snaphash_mode, data, z)


def run_dense(n, seed):
    """Data whose RLE1 form is exactly n bytes, dense in runs of 1-300, with a count byte of 0 (a run of 4) and one of
    251 (a run of 255) placed first in a few chunks."""
    r = random.Random(seed)
    cs = chunk_of(n)
    nch = -(-n // cs)
    parts, prev, enc = [], -1, 0

    def put(run):
        nonlocal prev, enc
        v = r.randrange(255)
        v += v >= prev
        parts.append(bytes([v]) * run)
        prev, enc = v, enc + rle1_len(run)

    def fill_to(target):  # random runs, then single bytes, up to exactly `target` RLE1 bytes
        while enc < target - 11:
            put(r.randrange(1, 301))
        while enc < target:
            put(1)

    for k, run in ((3, 4), (5, 255), (nch // 2, 4), (nch - 3, 255)):
        fill_to(k * cs - 4)  # the run's four bytes end the chunk before, its count starts chunk k
        put(run)
    fill_to(n)
    return b"".join(parts)


@pytest.mark.parametrize("n,lv", [(20000, 1), (65536, 1), (99981, 1), (899981, 9)])
def test_rle1_chunk_boundaries(snaphash_mode, n, lv):
    data = run_dense(n, n)
    pre = rle1(data)
    assert len(pre) == n
    cs, entries = chunk_entries(pre)
    assert cs == (64 if n <= 65536 else {99981: 98, 899981: 879}[n])
    assert {s for s, _ in entries} == {0, 1, 2, 3, 4}, "an RLE1 entry state occurs at no chunk boundary"
    assert (4, 0) in entries and (4, 251) in entries, "no count byte of 0 or 251 first in a chunk"
    with Context(device=0) as c:
        decode_one_block(c, snaphash_mode, data, bz2.compress(data, lv))


def test_the_host_suites_edges(snaphash_mode):
    """The inputs of test_bzip2_host.py's test_rle1_edges, test_every_level_and_every_byte_value and
    test_concatenated_streams_of_different_levels, on the kernels."""
    with Context(device=0) as c:
        r = random.Random(3)
        for k in (1, 2, 3, 4, 5, 6, 7, 8, 9, 255, 256, 257, 258, 259, 260, 1000, 4096):
            for v in (0, 0x41, 0xff):
                d = bytes([v]) * k
                assert c.bunzip2_buffer(bz2.compress(d, 9)) == d, (k, v)
                d2 = b"ab" + bytes([v]) * k + b"c" + bytes([v ^ 1]) * (k + 1)
                z = bz2.compress(d2, 1)
                assert c.bunzip2_buffer(z) == d2, (k, v)
                check_stats(c, snaphash_mode, d2, z)
        parts = []
        for _ in range(3000):
            parts.append(bytes([r.randrange(4)]) * r.choice([1, 2, 3, 4, 5, 8, 250, 259, 300]))
        d = b"".join(parts)
        for lv in (1, 9):
            assert c.bunzip2_buffer(bz2.compress(d, lv)) == d
        d = text(400000, 1) + bytes(range(256)) * 40 + bytes(range(255, -1, -1)) * 7
        for lv in range(1, 10):
            z = bz2.compress(d, lv)
            assert c.bunzip2_buffer(z) == d, lv
            check_stats(c, snaphash_mode, d, z)
        a, b, e = text(250000, 7), bytes(range(256)) * 900, text(1300000, 8)
        z = bz2.compress(a, 1) + bz2.compress(b, 5) + bz2.compress(e, 9)
        assert bz2.decompress(z) == a + b + e
        assert c.bunzip2_buffer(z) == a + b + e
        check_stats(c, snaphash_mode, a + b + e, z)
        assert c.bunzip2_buffer(bz2.compress(b"", 3) + bz2.compress(a, 2)) == a


def test_periodic_stream_between_ordinary_ones(snaphash_mode):
    a, p, q, b = text(300000, 30), bytes(255 * 3529), periodic_unit(16, 31) * 6000, run_free(50000, 32)
    z = bz2.compress(a, 9) + bz2.compress(p, 9) + bz2.compress(q, 1) + bz2.compress(b, 1)
    assert bz2.decompress(z) == a + p + q + b
    with Context(device=0) as c:
        assert c.bunzip2_buffer(z) == a + p + q + b
        st = check_stats(c, snaphash_mode, a + p + q + b, z)
        assert st["segments"] == 4, st


def test_unpack_with_a_periodic_member_stream(snaphash_mode, tmp_path, umask_022):  # noqa: F811
    """A tar whose bzip2 form is three streams, the middle one exactly a member's 255 * m zero bytes (one periodic
    block): tar_unpack_bz2 with hashes.yaml must verify it and write the tree the .gz path writes."""
    m = 3529
    build = make_tree(str(tmp_path))
    zp = os.path.join(build, "share", "zeros255")
    with open(zp, "wb") as f:
        f.write(bytes(255 * m))
    os.chmod(zp, 0o644)
    arc_gz, arc_bz = str(tmp_path / "data.tar.gz"), str(tmp_path / "data.tar.bz2")
    with Context(device=0) as c:
        yaml, _ = c.tar_create(arc_gz, build, build + "/DEBIAN", with_hashes=True)
        raw = gzip.decompress(open(arc_gz, "rb").read())
        with tarfile.open(fileobj=io.BytesIO(raw)) as t:
            mem = next(x for x in t.getmembers() if x.name.endswith("share/zeros255"))
        a, b = mem.offset_data, mem.offset_data + mem.size
        assert raw[a:b] == bytes(255 * m)
        mid = bz2.compress(raw[a:b], 9)
        assert len(rle1(raw[a:b])) == 5 * m
        with open(arc_bz, "wb") as f:
            f.write(bz2.compress(raw[:a], 9) + mid + bz2.compress(raw[b:], 9))
        assert bz2.decompress(open(arc_bz, "rb").read()) == raw
        decode_one_block(c, snaphash_mode, raw[a:b], mid)
        mis, _ = c.tar_unpack_bz2(arc_bz, str(tmp_path / "bz"), _yaml_for(yaml, arc_bz))
        assert mis is None
        if snaphash_mode == "gpu_only":
            st = c.unpack_stats()
            assert st["gpu_segments"] == st["segments"] and st["host_bytes"] == 0, st
        assert c.tar_unpack(arc_gz, str(tmp_path / "gz"), yaml)[0] is None
    assert tree_view(str(tmp_path / "bz")) == tree_view(str(tmp_path / "gz"))


def test_header_level_below_the_block_size(snaphash_mode):
    """A level-9 block of more than 100 000 symbols under a BZh1 header: libbz2 refuses it, and so must the decoder."""
    d = run_free(150000, 40)
    z = bz2.compress(d, 9)
    assert len(rle1(d)) == 150000
    bad = b"BZh1" + z[4:]
    with pytest.raises((OSError, ValueError)):
        bz2.decompress(bad)
    with Context(device=0) as c:
        with pytest.raises(_lib.SnaphashError) as e:
            c.bunzip2_buffer(bad)
        assert e.value.code == _lib.EFORMAT
        assert c.bunzip2_buffer(z) == d
