"""The CRC-64/XZ kernels (snappy_amd/csrc/crc_kernels.hip, crc_core.h) at their edges: snaphash_crc64_device against the
bitwise routine of tests/xz_cases.py, as tests/test_gpu_crc_edges.py does for CRC-32 -- every short length, every start
and end alignment, the lengths around a lane's 256-byte slice and a workgroup's 64 KiB tile, many ranges in one call,
empty and overlapping ranges, and canary words around the result array."""
import ctypes

import numpy as np
import pytest

import xz_cases as X

pytestmark = [pytest.mark.gpu, pytest.mark.kernels_only("the kernels are the same in both configurations")]

N = 1 << 18
SLICE, TILE = 256, 1 << 16


@pytest.fixture(scope="module")
def c64(built_lib):
    from snappy_amd import Context, _lib
    with Context(flags=_lib.FLAG_GPU_ONLY) as c:
        yield c


@pytest.fixture(scope="module")
def buf():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    host = np.random.default_rng(11).integers(0, 256, N, dtype=np.uint8)
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    return host.tobytes(), dev


_want = {}


def want(data, o, n):
    if (o, n) not in _want:
        _want[(o, n)] = X.crc64(data[o:o + n]) if n <= 700 else X.crc64_fast(data[o:o + n])
    return _want[(o, n)]


def check(c, buf, ranges):
    data, dev = buf
    assert dev.data_ptr() % 16 == 0 and all(o + n <= len(data) for o, n in ranges)
    offs = np.array([o for o, _ in ranges], dtype=np.uint64)
    lens = np.array([n for _, n in ranges], dtype=np.uint64)
    got = c.crc64_device(dev.data_ptr(), offs, lens).tolist()
    bad = [(o, n, hex(g), hex(want(data, o, n))) for (o, n), g in zip(ranges, got) if g != want(data, o, n)]
    assert not bad, bad[:5]


def test_lengths_0_to_600(c64, buf):
    check(c64, buf, [(0, n) for n in range(601)])


def test_every_alignment_at_both_ends(c64, buf):
    check(c64, buf, [(a, 1000 - a + b) for a in range(16) for b in range(16)])


def test_slice_and_tile_neighbours(c64, buf):
    lens = [SLICE - 1, SLICE, SLICE + 1, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 1, 3 * TILE + 5]
    check(c64, buf, [(0, n) for n in lens] + [(3, n) for n in lens])


def test_1024_ranges_empty_and_overlapping(c64, buf):
    rng = np.random.default_rng(12)
    ranges = []
    for i in range(1024):
        if i % 5 == 1:
            ranges.append((int(rng.integers(0, N)), 0))
        else:
            n = int(rng.integers(1, 700))
            ranges.append((int(rng.integers(0, N - n)), n))
    ranges[10] = (1000, TILE + 700)  # two ranges that overlap, one of them of two tiles
    ranges[11] = (1500, TILE + 100)
    ranges[1023] = (N - 1, 1)        # the buffer's last byte
    check(c64, buf, ranges)


def test_nothing_is_written_around_the_result(c64, buf):
    from snappy_amd import _lib
    _, dev = buf
    n = 7
    offs = np.arange(n, dtype=np.uint64) * 1000
    lens = np.full(n, 999, dtype=np.uint64)
    out = np.full(n + 8, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    rc = _lib.lib().snaphash_crc64_device(c64._h, dev.data_ptr(), offs.ctypes.data, lens.ctypes.data, n, out[4:].ctypes.data)
    assert rc == 0
    assert (out[:4] == 0xA5A5A5A5A5A5A5A5).all() and (out[4 + n:] == 0xA5A5A5A5A5A5A5A5).all()
    assert out[4:4 + n].tolist() == [want(buf[0], int(o), 999) for o in offs]
    assert len(c64.crc64_device(dev.data_ptr(), offs[:0], lens[:0])) == 0
