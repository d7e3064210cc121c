"""crc_ranges_kernel / crc_fold_kernel (snappy_amd/csrc/crc_kernels.hip) at their own edges, through
snaphash_crc32_device against the Python oracle (tests/crc_oracle.py: zlib.crc32, and a table CRC held against libbz2):
short lengths around the 16-byte loads, a lane's slice, one, two and three tiles with their neighbours, every start
alignment, many ranges in one call with empty and overlapping ones, buffers of random bytes, zeros and 0xFF.  One launch
per test and flavour.  The entry point never plans, so both configurations would run the same code: GPU-only alone."""
import numpy as np
import pytest

import crc_oracle
from crc_oracle import BZIP2, GZIP

pytestmark = [pytest.mark.gpu, pytest.mark.kernels_only("the CRC kernels themselves: the entry point has no planned form")]

TILE, SLICE = 65536, 256  # crc_core.h: kCrcTile, kCrcSlice (tests/test_crc_host.py reads them from the header)
KINDS = [GZIP, BZIP2]
N = 3 * TILE + 5 + 64


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def crc_ctx(built_lib):
    from snappy_amd import Context, _lib
    with Context(flags=_lib.FLAG_GPU_ONLY) as c:
        yield c


@pytest.fixture(scope="module")
def bufs():
    """name -> (host bytes, device tensor); the device copy starts 16-byte aligned (torch's allocator gives 256)."""
    torch = _torch()
    crc_oracle.check_bz_oracle()
    host = {"random": np.random.default_rng(3).integers(0, 256, N, dtype=np.uint8),
            "zeros": np.zeros(N, dtype=np.uint8), "ff": np.full(N, 0xFF, dtype=np.uint8)}
    out = {k: (v.tobytes(), torch.from_numpy(v).cuda()) for k, v in host.items()}
    torch.cuda.synchronize()
    return out


_want = {}


def want(kind, name, data, off, n):
    key = (kind, name, off, n)
    if key not in _want:
        _want[key] = crc_oracle.crc(kind, data[off:off + n])
    return _want[key]


def check(c, kind, bufs, name, ranges):
    data, dev = bufs[name]
    assert dev.data_ptr() % 16 == 0
    assert all(o + n <= len(data) for o, n in ranges)
    offs = np.array([o for o, _ in ranges], dtype=np.uint64)
    lens = np.array([n for _, n in ranges], dtype=np.uint64)
    got = c.crc32_device(kind, dev.data_ptr(), offs, lens)
    bad = [(o, n, hex(g), hex(want(kind, name, data, o, n))) for (o, n), g in zip(ranges, got.tolist()) if g != want(kind, name, data, o, n)]
    assert not bad, bad[:5]


@pytest.mark.parametrize("kind", KINDS)
def test_short_lengths(crc_ctx, bufs, kind):
    check(crc_ctx, kind, bufs, "random", [(0, n) for n in (0, 1, 2, 3, 4, 15, 16, 17, 31, 32, 33)])


@pytest.mark.parametrize("kind", KINDS)
def test_slice_and_tile_neighbours(crc_ctx, bufs, kind):
    lens = [SLICE - 1, SLICE, SLICE + 1, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 3 * TILE + 5]
    check(crc_ctx, kind, bufs, "random", [(0, n) for n in lens] + [(3, n) for n in lens])


@pytest.mark.parametrize("kind", KINDS)
def test_start_offsets(crc_ctx, bufs, kind):
    check(crc_ctx, kind, bufs, "random", [(o, 1000) for o in range(17)])


@pytest.mark.parametrize("kind", KINDS)
def test_many_ranges_empty_and_overlapping(crc_ctx, bufs, kind):
    rng = np.random.default_rng(9)
    ranges = []
    for i in range(300):
        if i % 3 == 1:
            ranges.append((int(rng.integers(0, N)), 0))  # an empty range between non-empty ones
        else:
            n = int(rng.integers(1, 3000))
            ranges.append((int(rng.integers(0, N - n)), n))
    ranges[10] = (1000, TILE + 700)   # two ranges that overlap, one of them of two tiles
    ranges[11] = (1500, TILE + 100)
    ranges[299] = (N - 1, 1)          # the buffer's last byte
    check(crc_ctx, kind, bufs, "random", ranges)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["zeros", "ff"])
def test_constant_buffers(crc_ctx, bufs, kind, name):
    check(crc_ctx, kind, bufs, name, [(0, 0), (1, 1), (5, 33), (7, SLICE + 1), (0, TILE), (9, TILE + 1), (1, 3 * TILE + 5)])


def test_bad_arguments(crc_ctx, bufs):
    from snappy_amd import SnaphashError
    _, dev = bufs["random"]
    one = np.array([0], dtype=np.uint64)
    with pytest.raises(SnaphashError):
        crc_ctx.crc32_device(2, dev.data_ptr(), one, one)
    assert len(crc_ctx.crc32_device(GZIP, dev.data_ptr(), one[:0], one[:0])) == 0
