"""The .bz2 writer's kernels at their own edges, stage by stage: bz_enc_rle1_kernel, bz_enc_bwt_kernel, bz_enc_mtf_kernel,
bz_enc_code_kernel and bz_enc_concat_kernel through snaphash_bzenc_stages_device -- the producer's sequence for a staged
slot, step for step, over the caller's ranges -- on device buffers of 0xA5 with 4 KiB of canary on both sides, every array
held whole against the host model's (tests/bz2enc_stage_model.h be_stages, which test_bz2enc_host.py ties to the model's
file and to plain Python references of RLE1, the BWT and MTF): RLE1's bytes, the last column, the symbols, the used-byte
map, the selectors, every slot word, every result and place, every word of the output, and the fill behind each stage's
length.  test_gpu_bz2enc.py compares finished files only: a write that lands where the next stage never reads -- block b's
scratch is followed directly by block b + 1's -- is invisible there, and nothing there says which stage went wrong.
The inputs are bz2enc_cases.edge_cases(), chosen for how the kernels cut the work (RLE1's 1024-lane tiles and its
lookahead, MTF's 64-symbol tiles and list positions through the from_last mode, the coding kernel's groups a lane, concat's
bit offsets and sweeps), and cases() at level 1.  The guard cases give one block more RLE1 output than a small cap holds:
the call fails as the producer would, and a store without its check would land in the canary or in a neighbour's fill.
NOT reachable through the entry, whose own refusals come first: MTF's `at < room`, BzW.over and the coding kernel's
selector-count check."""
import bz2

import numpy as np
import pytest

import bz2enc_cases as B
from snappy_amd import Context, _lib
from test_bz2enc_host import (ARRAYS, FILL, GUARD_OUT_WORDS, MAP_BYTES, RES_WORDS, SEL_STRIDE, edges_of, encode, finish, load_model, pieces_edge,
                              put_columns, read_slot, stage_counts, stages)

pytestmark = [pytest.mark.gpu, pytest.mark.kernels_only("names FLAG_GPU_ONLY itself")]

CANARY = 4096
IMPOSSIBLE = "bzip2: a block's stages reported an impossible result"


@pytest.fixture(scope="module")
def be():
    return load_model()


@pytest.fixture(scope="module")
def kctx(built_lib):
    with Context(device=0, flags=_lib.FLAG_GPU_ONLY) as c:
        yield c


@pytest.fixture(scope="module")
def model(be):
    """Edge -> the model's arrays: computed once an input and left alone."""
    cache = {}

    def get(e):
        if e.name not in cache:
            cache[e.name] = stages(be, e)
        return cache[e.name]
    return get


def edge(be, name):
    return next(e for e in edges_of(be) if e.name == name)


def device_stages(c, be, e, want, fails=False):
    """The entry over one Edge in fresh device buffers of FILL (slots, res and out too: the launchers are to zero them);
    -> the nine arrays, canaries checked and cut off.  The input stands between canaries as well and must not change."""
    import torch
    cap, nblk = want["cap"], want["nblk"]
    out_words = len(want["out"])
    cnt = stage_counts(be, nblk, cap, out_words)
    nbytes = {k: cnt[k] * np.dtype(dt).itemsize for k, dt in ARRAYS}
    bufs = {k: torch.full((nbytes[k] + 2 * CANARY,), FILL, dtype=torch.uint8, device="cuda") for k, _ in ARRAYS}
    ptrs = [bufs[k].data_ptr() + CANARY for k, _ in ARRAYS]
    if e.kind == "last":
        h = np.full(nbytes["last"] + 2 * CANARY, FILL, dtype=np.uint8)
        put_columns(h[CANARY:], e.columns, cap)
        bufs["last"].copy_(torch.from_numpy(h))
        meta = tuple(np.array([f(col) for col in e.columns], dtype=np.uint32) for f in (lambda t: len(t[0]), lambda t: t[1], lambda t: t[2]))
        args = (0, None, None, e.level, e.cap, e.carry, e.carry_bits, ptrs, out_words, meta)
    else:
        h_in = np.full(len(e.data) + 2 * CANARY, FILL, dtype=np.uint8)
        h_in[CANARY:CANARY + len(e.data)] = np.frombuffer(e.data, dtype=np.uint8)
        d_in = torch.from_numpy(h_in).cuda()
        offs = np.array([o for o, _ in e.ranges], dtype=np.uint64)
        lens = np.array([n for _, n in e.ranges], dtype=np.uint64)
        args = (d_in.data_ptr() + CANARY, offs, lens, e.level, e.cap, e.carry, e.carry_bits, ptrs, out_words)
    torch.cuda.synchronize()
    if fails:
        with pytest.raises(_lib.SnaphashError) as err:
            c.bzenc_stages_device(*args)
        assert err.value.code == _lib.EDEVICE and IMPOSSIBLE in str(err.value), e.name
        total = -1
    else:
        total = c.bzenc_stages_device(*args)
    got = {"total": total}
    for k, dt in ARRAYS:
        h = bufs[k].cpu().numpy()
        assert (h[:CANARY] == FILL).all() and (h[CANARY + nbytes[k]:] == FILL).all(), "%s: the canary around d_%s" % (e.name, k)
        got[k] = h[CANARY:CANARY + nbytes[k]].copy().view(dt)
    if e.kind != "last":
        assert np.array_equal(d_in.cpu().numpy(), h_in), "%s: the input changed" % e.name
    return got


def same_as_model(got, want, what):
    """Every array whole; of a block whose RLE1 output exceeded cap only what RLE1 leaves (its bytes, rle_n 0, over 1):
    the later stages' arrays are not stated inside that block's own strides."""
    nblk, room = want["nblk"], want["cap"] + 64
    stride = {"rle": room, "last": room, "syms": room, "maps": MAP_BYTES, "sel": SEL_STRIDE, "slots": len(want["slots"]) // max(nblk, 1),
              "res": RES_WORDS, "dst": 1, "out": 0}
    for k, _ in ARRAYS:
        g, w = got[k], want[k]
        assert len(g) == len(w), (what, k)
        differs = g != w
        for b in np.flatnonzero(want["over"]):
            if k in ("last", "syms", "maps", "sel", "slots"):
                differs[b * stride[k]:(b + 1) * stride[k]] = False
            elif k == "res":
                differs[b * RES_WORDS + 1:b * RES_WORDS + 4] = False  # orig_ptr, nmtf, bits
        if differs.any():
            at = int(np.flatnonzero(differs)[0])
            raise AssertionError("%s: d_%s differs from the model's at index %d (block %d): %#x, not %#x (%d places in all)"
                                 % (what, k, at, at // stride[k] if stride[k] else 0, int(g[at]), int(w[at]), int(differs.sum())))
    assert got["total"] == want["total"], what
    over = got["res"][4::RES_WORDS]
    assert over.tolist() == want["over"].tolist(), (what, "res.over")


def check_edge(c, be, e, want, what=None):
    what = what or e.name
    got = device_stages(c, be, e, want, fails=e.kind == "guard")
    same_as_model(got, want, what)
    sw = len(got["slots"]) // want["nblk"]
    slots = [read_slot(be, got["slots"][k * sw:(k + 1) * sw], want["cap"]) for k in range(want["nblk"]) if not want["over"][k]]
    if e.kind == "last":  # the slot's bits read back to exactly what was given
        for k, (st, col, op, crc, end) in enumerate(slots):
            assert (st, col, op, crc) == (0,) + tuple(e.columns[k]) and end == int(got["res"][k * RES_WORDS + 3]), (what, k)
    elif e.kind == "pieces":  # the host finishes the file from d_out: libbz2 gives back the ranges' bytes in order
        z = finish(e.level, got["out"], got["total"], [s[3] for s in slots], e.carry_bits)
        assert bz2.decompress(z) == b"".join(e.data[o:o + n] for o, n in e.ranges), what
        return z
    return None


@pytest.mark.parametrize("name", B.edge_names())
def test_every_stage_equals_the_model_at_the_edges(kctx, be, model, name):
    e = edge(be, name)
    check_edge(kctx, be, e, model(e))


@pytest.mark.parametrize("name", [n for n, _ in B.cases()])
def test_every_stage_equals_the_model_on_the_producers_pieces(kctx, be, model, name):
    data = dict(B.cases())[name]
    if not data:  # no block: nothing to launch, the bit behind the carry
        assert kctx.bzenc_stages_device(0, np.zeros(0, np.uint64), np.zeros(0, np.uint64), 1, 0, 0x80, 1, [0] * 9, 0) == 1
        return
    e = pieces_edge(name, data, 1)
    assert check_edge(kctx, be, e, model(e)) == encode(be, data, 1)[0], name


def test_the_arrays_do_not_depend_on_what_the_ctx_did_before(be, model, built_lib):
    """The same input twice in one ctx, after a different input, and across levels: level 9 makes the ctx's sort scratch
    larger than level 1 needs, and level 9 comes after level 1 allocated for less."""
    tiles, cat, fib = edge(be, "rle1_tile_edges"), edge(be, "concat_%d_blocks_carry_7" % B.CONCAT_BLOCKS), edge(be, "fibonacci_level9")
    l1 = pieces_edge("six_pieces", dict(B.cases())["six_pieces"], 1)
    with Context(device=0, flags=_lib.FLAG_GPU_ONLY) as c:
        for n, e in enumerate((tiles, tiles, cat, tiles, l1, fib, l1, tiles, fib, edge(be, "front_runs"), cat)):
            check_edge(c, be, e, model(e), "%s as call %d of one ctx" % (e.name, n))


def test_the_entry_refuses_what_it_cannot_do(kctx, be, model):
    import torch
    e = edge(be, "guard_exactly_cap")
    want = model(e)
    cap, nblk, out_words = want["cap"], want["nblk"], len(want["out"])
    cnt = stage_counts(be, nblk, cap, out_words)
    bufs = {k: torch.full((cnt[k] * np.dtype(dt).itemsize,), FILL, dtype=torch.uint8, device="cuda") for k, dt in ARRAYS}
    ptrs = [bufs[k].data_ptr() for k, _ in ARRAYS]
    d_in = torch.frombuffer(bytearray(e.data), dtype=torch.uint8).cuda()
    offs = np.array([o for o, _ in e.ranges], dtype=np.uint64)
    lens = np.array([n for _, n in e.ranges], dtype=np.uint64)
    rn = np.array([int(want["res"][k * RES_WORDS]) for k in range(nblk)], dtype=np.uint32)
    op = np.array([int(want["res"][k * RES_WORDS + 1]) for k in range(nblk)], dtype=np.uint32)
    crc = np.arange(nblk, dtype=np.uint32)
    torch.cuda.synchronize()

    def refused(*args, **kw):
        with pytest.raises(_lib.SnaphashError) as err:
            kctx.bzenc_stages_device(*args, **kw)
        assert err.value.code == _lib.EINVAL, (args, kw)

    def changed(a, k, v):
        a = a.copy()
        a[k] = v
        return a

    good = (d_in.data_ptr(), offs, lens, 1, cap, 0, 0, ptrs, out_words)
    refused(*good[:2], changed(lens, 2, 0), *good[3:])                      # a length of 0
    refused(*good[:2], changed(lens, 2, B.PIECE + 1), *good[3:])            # above the piece
    for level in (0, 10, 1 << 31):
        refused(*good[:3], level, *good[4:])
    for bad_cap in (1, 63, 65, 1000, 899840 + 64, 0xffffffc0):
        refused(*good[:4], bad_cap, *good[5:])
    refused(*good[:5], 0x80, 0, *good[7:])                                  # carry bits that carry_bits does not cover
    refused(*good[:5], 0, 8, *good[7:])
    refused(0, *good[1:])
    for i in range(len(ptrs)):                                              # null arrays
        refused(*good[:7], ptrs[:i] + [0] + ptrs[i + 1:], out_words)
    last = (0, None, None, 1, cap, 0, 0, ptrs, out_words)
    refused(*last, from_last=(changed(rn, 1, 0), op, crc))                  # rle_n of 0, above cap
    refused(*last, from_last=(changed(rn, 1, cap + 1), op, crc))
    refused(*last, from_last=(rn, changed(op, 3, rn[3]), crc))              # orig_ptr >= rle_n
    for k, _ in ARRAYS:  # refused before anything is launched: nothing was written
        assert (bufs[k].cpu().numpy() == FILL).all(), k
    refused(*good[:8], out_words - 1)                                       # too small for the placed bits, once they are known
    assert (bufs["dst"].cpu().numpy() == FILL).all() and (bufs["out"].cpu().numpy() == FILL).all()
    # the ctx still works: the entry, and the producer
    check_edge(kctx, be, e, want, "after the refusals")
    data = dict(B.cases())["text_%d" % (B.PIECE + 1)]
    assert kctx.bzip2_buffer(data, 1) == encode(be, data, 1)[0]
