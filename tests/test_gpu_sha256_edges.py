"""sha256_ranges_kernel (snappy_amd/csrc/sha256_kernels.hip, sha256_core.h) at its edges: snaphash_sha256_device against
hashlib.sha256, laid out as tests/test_gpu_crc64_edges.py is -- every short length, every start and end alignment, the
lengths around the kernel's own units, a full wave of ranges and one lane more, many ranges with empty and overlapping ones,
ranges of very unequal length (the host sorts them by block count: every digest must still come back at its own index),
and canary bytes around the result array."""
import hashlib

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.kernels_only("the kernel is the same in both configurations")]

N = 1 << 18
# the kernel's units (sha256_core.h): a block, the 16-byte load, the step the prefetch runs ahead by, a range's tile row
BLOCK, LOAD, STEP, TILE_ROW = 64, 16, 64, 80
WAVE = 64


@pytest.fixture(scope="module")
def c256(built_lib):
    from snappy_amd import Context, _lib
    with Context(flags=_lib.FLAG_GPU_ONLY) as c:
        yield c


@pytest.fixture(scope="module")
def buf():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    host = np.random.default_rng(256).integers(0, 256, N, dtype=np.uint8)
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    return host.tobytes(), dev


_want = {}


def want(data, o, n):
    if (o, n) not in _want:
        _want[(o, n)] = hashlib.sha256(data[o:o + n]).digest()
    return _want[(o, n)]


def check(c, buf, ranges):
    data, dev = buf
    assert dev.data_ptr() % 16 == 0 and all(o + n <= len(data) for o, n in ranges)
    offs = np.array([o for o, _ in ranges], dtype=np.uint64)
    lens = np.array([n for _, n in ranges], dtype=np.uint64)
    got = c.sha256_device(dev.data_ptr(), offs, lens)
    assert got.shape == (len(ranges), 32) and got.dtype == np.uint8
    bad = [(i, o, n) for i, (o, n) in enumerate(ranges) if got[i].tobytes() != want(data, o, n)]
    assert not bad, bad[:5]


def test_units_are_the_kernels():
    """The constants this file names are the ones the kernel is built from."""
    from test_sha256_host import load_sha
    L = load_sha()
    assert (L.sh_block_bytes(), L.sh_load_bytes(), L.sh_step_bytes(), L.sh_tile_row_bytes()) == (BLOCK, LOAD, STEP, TILE_ROW)


def test_lengths_0_to_600(c256, buf):
    check(c256, buf, [(0, n) for n in range(601)])


def test_every_alignment_at_both_ends(c256, buf):
    check(c256, buf, [(a, 1000 - a + b) for a in range(16) for b in range(16)])


def test_unit_neighbours(c256, buf):
    lens = set()
    for unit in (LOAD, BLOCK, STEP, 2 * STEP, 3 * STEP, TILE_ROW, 2 * TILE_ROW):
        lens |= {unit - 9, unit - 8, unit - 1, unit, unit + 1}  # (- 9 / - 8: where the bit length stops fitting)
    lens = sorted(lens) + [65535, 65536, 65537]
    check(c256, buf, [(0, n) for n in lens] + [(3, n) for n in lens] + [(13, n) for n in lens] + [(0, N)])


@pytest.mark.parametrize("count", [WAVE, WAVE + 1, 2 * WAVE + 1])
def test_full_wave_and_one_lane_more(c256, buf, count):
    check(c256, buf, [(7 * i, 100 + 3 * i) for i in range(count)])


def test_1024_ranges_empty_and_overlapping(c256, buf):
    rng = np.random.default_rng(12)
    ranges = []
    for i in range(1024):
        if i % 5 == 1:
            ranges.append((int(rng.integers(0, N)), 0))
        else:
            n = int(rng.integers(1, 700))
            ranges.append((int(rng.integers(0, N - n)), n))
    ranges[10] = (1000, 5000)  # two ranges that overlap
    ranges[11] = (1500, 4100)
    ranges[1023] = (N - 1, 1)  # the buffer's last byte
    check(c256, buf, ranges)


def test_unequal_lengths_keep_their_index(c256, buf):
    """1 byte beside 200 KiB: the host's sort by block count moves them apart, the digests come back where they belong."""
    ranges = [(5, 1), (11, 200 << 10), (0, 0), (100, 64), (3, 50_000), (9, 1), (N - 70_000, 70_000), (17, 2)]
    ranges += [(i, 1 + (i * 37) % 300) for i in range(70)]  # a second wave's worth, so the long ones change waves too
    check(c256, buf, ranges)
    check(c256, buf, ranges[::-1])


def test_nothing_is_written_around_the_result(c256, buf):
    from snappy_amd import _lib
    _, dev = buf
    n = 7
    offs = np.arange(n, dtype=np.uint64) * 1000 + 3
    lens = np.full(n, 999, dtype=np.uint64)
    out = np.full((n + 2) * 32, 0xA5, dtype=np.uint8)
    rc = _lib.lib().snaphash_sha256_device(c256._h, dev.data_ptr(), offs.ctypes.data, lens.ctypes.data, n, out[32:].ctypes.data)
    assert rc == 0
    assert (out[:32] == 0xA5).all() and (out[32 + 32 * n:] == 0xA5).all()
    assert [out[32 + 32 * i:64 + 32 * i].tobytes() for i in range(n)] == [want(buf[0], int(o), 999) for o in offs]


def test_no_ranges(c256, buf):
    _, dev = buf
    empty = np.zeros(0, dtype=np.uint64)
    got = c256.sha256_device(dev.data_ptr(), empty, empty)
    assert got.shape == (0, 32)
