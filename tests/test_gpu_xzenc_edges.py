"""The .xz writer's kernels at their own edges, stage by stage: lzma_chains_kernel, lzma2_chunks_kernel and
lzma2_concat_kernel through snaphash_xzenc_stages_device -- the producer's sequence for a staged piece, step for step -- on
device buffers of 0xA5 with 4 KiB of canary on both sides, every array held whole against the host model's
(tests/xzenc_host_harness.cpp xe_stages, which test_xzenc_host.py ties to the model's file): the chains and the
candidates at every position, every chunk's result and place, every slot byte (what does not fit is counted and not
stored; a chunk that gives up leaves the same partial bytes) and every byte of the output (nothing in the room left for
Block headers, padding and Checks, nothing behind the last Block).  test_gpu_xzenc.py compares final files only: a
write that lands where the next stage never reads is invisible there.  The file the host makes of the kernels' output
goes to liblzma.  The chunk launches are cut at widths that put one Block's chunks into two launches (the producer's
own width, 2048 chunks, would take 128 MiB to do that), and far_dists sends one Block of 4 MiB, the largest, through
the entry and through snaphash_xz_buffer / snaphash_unxz_buffer."""
import lzma

import numpy as np
import pytest

import xz_cases as X
import xzenc_cases as E
from snappy_amd import Context, _lib
from test_xzenc_host import FILL, SLOT, encode, finish, load_enc, out_cap, stages

pytestmark = [pytest.mark.gpu, pytest.mark.kernels_only("names FLAG_GPU_ONLY itself")]

CANARY = 4096
ARRAYS = (("prev", np.uint32), ("cand", np.uint32), ("slots", np.uint8), ("res", np.uint32), ("dst", np.uint64), ("out", np.uint8))
WIDTHS = (1, 2, 3, 7, 0)


@pytest.fixture(scope="module")
def xe():
    return load_enc()


@pytest.fixture(scope="module")
def kctx(built_lib):
    with Context(device=0, flags=_lib.FLAG_GPU_ONLY) as c:
        yield c


@pytest.fixture(scope="module")
def model(xe):
    """(data, block size) -> (the model's arrays, the model's file): computed once an input and left alone."""
    cache = {}

    def get(data, bs):
        key = (data, bs)
        if key not in cache:
            rc, z = encode(xe, data, bs)
            assert rc == 0
            cache[key] = (stages(xe, data, bs), z)
        return cache[key]
    return get


def sizes(n):
    nch = (n + E.CHUNK - 1) // E.CHUNK
    return {"prev": 4 * n, "cand": 4 * n, "slots": nch * SLOT, "res": 4 * nch, "dst": 8 * nch, "out": out_cap(n)}


def device_stages(c, data, bs, width):
    """The entry over `data` in fresh device buffers of FILL; -> the six arrays (canaries checked and cut off) and the
    Blocks' totals."""
    import torch
    n = len(data)
    sz = sizes(n)
    bufs = {k: torch.full((sz[k] + 2 * CANARY,), FILL, dtype=torch.uint8, device="cuda") for k, _ in ARRAYS}
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if n else None
    torch.cuda.synchronize()
    total = c.xzenc_stages_device(d_in.data_ptr() if n else 0, n, bs, width, *(bufs[k].data_ptr() + CANARY for k, _ in ARRAYS), sz["out"])
    got = {}
    for k, dt in ARRAYS:
        h = bufs[k].cpu().numpy()
        assert (h[:CANARY] == FILL).all() and (h[CANARY + sz[k]:] == FILL).all(), "the canary around d_%s" % k
        got[k] = h[CANARY:CANARY + sz[k]].copy().view(dt)
    return got, total


def same_as_model(got, total, want, what):
    for k, _ in ARRAYS:
        if not np.array_equal(got[k], want[k]):
            at = int(np.flatnonzero(got[k] != want[k])[0])
            raise AssertionError("%s: d_%s differs from the model's at index %d: %#x, not %#x (%d places in all)"
                                 % (what, k, at, int(got[k][at]), int(want[k][at]), int((got[k] != want[k]).sum())))
    assert total == [int(t) for t in want["total"]], what


@pytest.mark.parametrize("name", [n for n, _, _ in E.cases()])
def test_every_stage_equals_the_model(kctx, xe, model, name):
    _, data, bs = E.by_name(name)
    want, z = model(data, bs)
    got, total = device_stages(kctx, data, bs, 0)
    same_as_model(got, total, want, name)
    mine = finish(xe, data, bs, got["res"], got["out"], sum(total))  # the host's part added to the kernels' bytes
    assert lzma.decompress(mine) == data and mine == z, name


def _width_inputs():
    seven = X.text(6 * E.CHUNK + 12345, 98)  # 7 chunks, the last one short
    out = [("text7_64k", seven, E.CHUNK), ("text7_128k", seven, 2 * E.CHUNK), ("text7_256k", seven, 4 * E.CHUNK)]
    for name in ("mixed_rtrt", "dist_edges"):  # dist_edges: matches that reach into chunks an earlier launch coded
        out.append(E.by_name(name))
    return out


@pytest.mark.parametrize("name", [n for n, _, _ in _width_inputs()])
def test_the_arrays_do_not_depend_on_the_launch_width(kctx, xe, model, name):
    """launch_chunks = 1, 2, 3, 7 and the producer's: chunk c0 + blockIdx.x of every launch, a last launch shorter than
    the width, and (256 KiB Blocks at width 3: chunks 0 1 2 | 3 4 5 | 6) Blocks whose chunks fall into two launches.
    NOT covered: launch_lzma2_chunks' refusal of a chunk behind the piece -- the entry, like the producer, never asks
    for more than nch - c0 chunks, so that check cannot fire through it."""
    _, data, bs = next(c for c in _width_inputs() if c[0] == name)
    assert len(data) > 3 * E.CHUNK
    want, z = model(data, bs)
    for w in WIDTHS:
        got, total = device_stages(kctx, data, bs, w)
        same_as_model(got, total, want, "%s at width %d" % (name, w))
        assert lzma.decompress(finish(xe, data, bs, got["res"], got["out"], sum(total))) == data, (name, w)


def test_a_block_of_4_mib_through_the_producer_and_the_install_side(kctx, model):
    """far_dists: distance slots up to 43, a candidate at the packing's limit, 65 536 tiles in one workgroup of the
    chains kernel (the entry runs it in test_every_stage_equals_the_model)."""
    _, data, bs = E.by_name("far_dists")
    assert len(data) == bs == 4 << 20
    z = kctx.xz_buffer(data, bs)
    assert z == model(data, bs)[1] and lzma.decompress(z) == data
    assert kctx.targz_stats()["chunks"] == 64 and kctx.targz_stats()["stored_chunks"] == 0
    assert kctx.unxz_buffer(z) == data
    st = kctx.unpack_stats()
    assert st["gpu_segments"] == st["segments"] == 1 and st["host_bytes"] == 0, st


def test_the_entry_refuses_what_it_cannot_do(kctx, xe, model):
    import torch
    _, data, bs = E.by_name("len_131073")
    n = len(data)
    sz = sizes(n)
    bufs = {k: torch.full((sz[k],), FILL, dtype=torch.uint8, device="cuda") for k, _ in ARRAYS}
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    ptrs = [bufs[k].data_ptr() for k, _ in ARRAYS]

    def refused(*args):
        with pytest.raises(_lib.SnaphashError) as e:
            kctx.xzenc_stages_device(*args)
        assert e.value.code == _lib.EINVAL, args

    for bad in (1, 65535, 65537, 3 * 65536 + 1, (4 << 20) + 65536, 1 << 40):
        refused(d_in.data_ptr(), n, bad, 0, *ptrs, sz["out"])
    refused(d_in.data_ptr(), n, bs, 2049, *ptrs, sz["out"])  # more than is resident at once
    refused(d_in.data_ptr(), n, bs, 0, *ptrs, sz["out"] - 1)
    refused(0, n, bs, 0, *ptrs, sz["out"])
    for i in range(len(ptrs)):
        refused(d_in.data_ptr(), n, bs, 0, *(ptrs[:i] + [0] + ptrs[i + 1:]), sz["out"])
    for k, _ in ARRAYS:  # a refusal has written nothing
        assert (bufs[k].cpu().numpy() == FILL).all(), k
    assert kctx.xzenc_stages_device(0, 0, bs, 0, 0, 0, 0, 0, 0, 0, 0) == []  # no bytes: nothing to do
    refused(0, 0, 65537, 0, 0, 0, 0, 0, 0, 0, 0)
    # the ctx still works: the entry at the widest launch it takes, and the producer
    got, total = device_stages(kctx, data, bs, 2048)
    same_as_model(got, total, model(data, bs)[0], "after the refusals")
    assert kctx.xz_buffer(data, bs) == model(data, bs)[1]
