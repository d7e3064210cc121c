"""lzma2_blocks_kernel at its own edges: every edge file of tests/xz_cases.py (the match distances and lengths at which
the wave copy can go wrong, every chunk kind, the properties at their bounds, 300 Blocks in one launch; test_xz_host.py
shows from the decoder's histogram that each shape occurs) through snaphash_unxz_buffer under FLAG_GPU_ONLY, with
gpu_segments == segments showing that the kernel decoded it and not the host fallback; and every Block of those files
once more through snaphash_unxz_block_device into a device buffer with canary bytes on both sides of the Block's range:
the byte-equality tests cannot see a copy that overruns into a neighbouring Block which is decoded later."""
import numpy as np
import pytest

import xz_cases as X
from snappy_amd import Context, _lib

pytestmark = [pytest.mark.gpu, pytest.mark.kernels_only("names FLAG_GPU_ONLY itself")]


@pytest.fixture(scope="module")
def kctx(built_lib):
    with Context(device=0, flags=_lib.FLAG_GPU_ONLY) as c:
        yield c


@pytest.mark.parametrize("name", [n for n, _, _ in X.edge_cases()])
def test_edge_file_through_the_kernel(kctx, name):
    z, plain = next((z, p) for n, z, p in X.edge_cases() if n == name)
    assert kctx.unxz_buffer(z) == plain
    st = kctx.unpack_stats()
    assert st["gpu_segments"] == st["segments"] >= 1 and st["host_bytes"] == 0, st


def test_a_block_the_kernel_refuses_is_refused_by_the_host_too(kctx):
    for name, z, _ in X.bad_cases():
        if name in ("flip_payload", "distance_beyond_produced", "control_03", "chunk_usize_minus_one", "first_chunk_no_dict_reset"):
            with pytest.raises(_lib.SnaphashError) as e:
                kctx.unxz_buffer(z)
            assert e.value.code == _lib.EFORMAT, name
    z, plain = next((z, p) for n, z, p in X.edge_cases() if n == "reps")
    assert kctx.unxz_buffer(z) == plain


CANARY = 4096


def _blocks_of(z, plain):
    """(index, uncompressed length, offset in plain) of every Block of a one-Stream file built by xz_cases: read from its Index."""
    import struct
    isize = (struct.unpack("<I", z[-8:-4])[0] + 1) * 4
    ix = z[len(z) - 12 - isize:len(z) - 12]
    at = 1

    def vli():
        nonlocal at
        v, sh = 0, 0
        while True:
            b = ix[at]
            at += 1
            v |= (b & 0x7F) << sh
            sh += 7
            if not b & 0x80:
                return v
    out, off = [], 0
    for i in range(vli()):
        vli()
        n = vli()
        out.append((i, n, off))
        off += n
    assert off == len(plain)
    return out


@pytest.mark.parametrize("name", [n for n, _, _ in X.edge_cases()])
def test_nothing_is_written_outside_a_blocks_range(kctx, name):
    """Each Block alone into the middle of a buffer of 0xA5: its bytes are right and the 4 KiB in front of it and behind
    it are untouched (a 64-lane copy or a 16-byte store that overran would land there)."""
    import torch
    z, plain = next((z, p) for n, z, p in X.edge_cases() if n == name)
    blocks = _blocks_of(z, plain)
    if len(blocks) > 8:  # of the 300 small Blocks: the first, the last and a few between
        blocks = blocks[:3] + blocks[150:152] + blocks[-3:]
    for i, n, off in blocks:
        dev = torch.full((n + 2 * CANARY,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        kctx.unxz_block_device(z, i, dev.data_ptr() + CANARY, n)
        got = dev.cpu().numpy()
        assert (got[:CANARY] == 0xA5).all() and (got[CANARY + n:] == 0xA5).all(), (name, i)
        assert got[CANARY:CANARY + n].tobytes() == plain[off:off + n], (name, i)


def test_block_device_refuses_what_it_cannot_do(kctx):
    import torch
    z, plain = next((z, p) for n, z, p in X.edge_cases() if n == "reps")
    dev = torch.zeros(len(plain) + 16, dtype=torch.uint8, device="cuda")
    for block, n in ((1, len(plain)), (0, len(plain) - 1), (0, len(plain) + 1)):
        with pytest.raises(_lib.SnaphashError) as e:
            kctx.unxz_block_device(z, block, dev.data_ptr(), n)
        assert e.value.code == _lib.EINVAL
    bad = next(zz for n, zz, _ in X.bad_cases() if n == "distance_beyond_produced")
    q_len = 3000 + 500 + 1000
    with pytest.raises(_lib.SnaphashError) as e:
        kctx.unxz_block_device(bad, 0, dev.data_ptr(), q_len)
    assert e.value.code == _lib.EFORMAT
