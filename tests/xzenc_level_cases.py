"""Inputs for the .xz writer's level (snappy_amd/csrc/xz_enc_core.h), shared by the CPU tests
(test_xzenc_level_host.py) and the GPU tests (test_gpu_xzenc_level.py), and the one place that loads
tests/xzenc_level_host_harness.cpp.  edge_cases() are made for what level 1 adds -- windows, candidates, prices -- at a
chunk's and a window's edges; the inputs of xzenc_cases.cases() are run at level 1 as well."""
import ctypes
import functools
import random

import numpy as np

import hostbuild
import xz_cases as X
import xzenc_cases as E

CHUNK = E.CHUNK
SLOT = CHUNK + 64
STORED = 0x80000000
KiB = 1024
MARGIN_KS = (64030, 64040, E.MARGIN_LZMA_K, E.MARGIN_STORED_K, E.MARGIN_GIVEUP_K, 64400, 65000)
# the harness's statistics
T_LIT, T_MATCHED_LIT, T_MATCH, T_REP, T_SHORT_REP, T_CROSSES, T_CODED, T_MAX_DIST, T_N = 0, 1, 2, 3, 7, 8, 9, 10, 11
OP_LIT, OP_SHORT_REP, OP_REP, OP_MATCH = 0, 1, 2, 3
P = ctypes.POINTER


def motifs(n, seed, count=300, size=24):
    """`count` motifs of `size` bytes repeated in random order.  They come in families of five that share their first 5, 9,
    13 or 17 bytes or all of them, so the chain of a position offers rising lengths, nearest first, wherever the nearer
    relative is the more distant one: most positions have several candidates, many all K, none of them maximal.  The paths
    never come together, so the windows run full and a match that would cross a window's end is cut there."""
    r = random.Random(seed)
    ms = []
    for _ in range(count // 5):
        base = r.randbytes(size)
        ms += [base] + [base[:5 + 4 * v] + r.randbytes(size - 5 - 4 * v) for v in range(4)]
    out = bytearray()
    while len(out) < n:
        out += r.choice(ms)
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def edge_cases():
    """[(name, bytes, block size)]: each a few hundred KiB at most, but far_dists' one 4 MiB Block."""
    out = []
    for k in (1, 2, 3):  # a Block's last chunk of k bytes
        out.append(("chunk_of_%d" % k, X.text(CHUNK + k, 200 + k), 2 * CHUNK))
    out.append(("run_over_chunk_end", X.text(CHUNK - 100, 204) + bytes([7]) * 300 + X.text(500, 205), 2 * CHUNK))
    out.append(("full_windows", motifs(2 * CHUNK + 777, 206), 4 * CHUNK))
    out.append(("zeros_273", X.text(300, 207) + bytes(1000) + X.text(500, 208) + bytes(600) + b"x" + bytes(273) + b"y" + bytes(274), CHUNK))
    out.append(("period_7", X.periodic(7, 70000), 2 * CHUNK))
    out.append(("period_300", X.periodic(300, 70000), 2 * CHUNK))
    out.append(("first_position", b"ab" * 50 + X.text(200, 209), CHUNK))
    out.append(("far_dists", E.far_dists()[0], E.FAR_BLOCK))
    out.append(("hash_twins", E.hash_twins(), E.B))
    out.append(("incompressible", X.rnd(2 * CHUNK + 100, 210), 2 * CHUNK))
    for k in MARGIN_KS:
        out.append(("margin_%d" % k, E.margin(k), CHUNK))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    """Every input the level is held to on both sides: xzenc_cases.cases() in Blocks of 64 KiB and 128 KiB (its 4 MiB
    far_dists Block as it is, once, among the edge cases), then the edge cases."""
    out = []
    for name, data, _ in E.cases():
        if name == "far_dists":
            continue
        for bs in (CHUNK, 2 * CHUNK):
            out.append(("%s@%dk" % (name, bs // KiB), data, bs))
    return out + list(edge_cases())


@functools.lru_cache(maxsize=None)
def load_level():
    """tests/xzenc_level_host_harness.cpp, loaded once a process with every prototype (it keeps no state between calls)."""
    L = hostbuild.shared("tests/xzenc_level_host_harness.cpp")
    vp, sz, u32, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint64
    L.xl_consts.argtypes = [P(u32)]
    L.xl_encode.argtypes = [ctypes.c_char_p, sz, u64, u32, ctypes.c_int, u32, P(sz), P(ctypes.c_int)]
    L.xl_encode.restype = vp
    L.xl_encode_plain.argtypes = [ctypes.c_char_p, sz, u64, P(sz), P(ctypes.c_int)]
    L.xl_encode_plain.restype = vp
    L.xl_free.argtypes = [vp]
    L.xl_ops.argtypes = [ctypes.c_char_p, sz, u64, u32, ctypes.c_int, P(u64), P(u32), sz, vp, sz, P(u64)]
    L.xl_ops.restype = ctypes.c_int64
    L.xl_stages.argtypes = [ctypes.c_char_p, sz, u64, u32, vp, vp, vp, vp, vp, vp, sz, vp]
    L.xl_stages.restype = ctypes.c_int64
    L.xl_chunk.argtypes = [ctypes.c_char_p, u32, vp, vp, ctypes.c_int, vp, vp, sz, P(u64)]
    L.xl_chunk.restype = u32
    L.xl_price_table.argtypes = [vp]
    L.xl_tables.argtypes = [vp, vp, vp, vp, vp, sz, vp, ctypes.c_char_p, vp]
    L.xl_find_set.argtypes = [ctypes.c_char_p, u32, u32, u32, vp]
    return L


def consts(L):
    """(K, W, depth, lanes)"""
    c = (ctypes.c_uint32 * 4)()
    L.xl_consts(c)
    return tuple(c)


def encode(L, data, block_size, level, descending=False, filter=0):
    """(rc, file) from the host model at a level."""
    n, rc = ctypes.c_size_t(), ctypes.c_int()
    p = L.xl_encode(data, len(data), block_size, level, int(descending), filter, ctypes.byref(n), ctypes.byref(rc))
    z = ctypes.string_at(p, n.value)
    L.xl_free(p)
    return rc.value, z


def encode_plain(L, data, block_size):
    n, rc = ctypes.c_size_t(), ctypes.c_int()
    p = L.xl_encode_plain(data, len(data), block_size, ctypes.byref(n), ctypes.byref(rc))
    z = ctypes.string_at(p, n.value)
    L.xl_free(p)
    return rc.value, z


def ops(L, data, block_size, level, descending=False, log=False):
    """(statistics, every chunk's result, the operations as rows of (kind, position, distance or k, length) or None)."""
    s = (ctypes.c_uint64 * T_N)()
    cap = len(data) // CHUNK + 2
    res = (ctypes.c_uint32 * cap)()
    n_ops = ctypes.c_uint64()
    rows = np.zeros((len(data) + 1, 4), np.uint32) if log else None
    n = L.xl_ops(data, len(data), block_size, level, int(descending), s, res, cap, rows.ctypes.data if log else None, len(data) + 1 if log else 0,
                 ctypes.byref(n_ops))
    assert 0 <= n <= cap
    return list(s), list(res[:n]), (rows[:n_ops.value] if log else None)


def chunk(L, blk, cand, probs=None, descending=False):
    """xzenc_chunk_priced over blk as one chunk with the caller's candidates (a (len(blk), K) uint32 array) and
    probabilities: (result, the operations)."""
    cand = np.ascontiguousarray(cand, np.uint32)
    assert cand.shape == (len(blk), consts(L)[0]) and len(blk) <= CHUNK
    out = np.zeros(SLOT, np.uint8)
    rows = np.zeros((len(blk) + 1, 4), np.uint32)
    n_ops = ctypes.c_uint64()
    pr = None if probs is None else np.ascontiguousarray(probs, np.uint16)
    r = L.xl_chunk(blk, len(blk), cand.ctypes.data, None if pr is None else pr.ctypes.data, int(descending), out.ctypes.data, rows.ctypes.data,
                   len(blk) + 1, ctypes.byref(n_ops))
    return r, rows[:n_ops.value]


def out_cap(n):
    """XzEncBufs::out_cap: what the Blocks of a piece of n bytes take at most."""
    return n + (n + CHUNK - 1) // CHUNK * 64 + 64


def stages(L, data, block_size, level, fill=0xA5):
    """The model stage by stage at a level, as the kernels leave their arrays (test_xzenc_host.stages with K candidate
    words a position at level 1): prev, cand, res, dst, slots, out, total, used."""
    n, bs = len(data), block_size or 1 << 20
    kw = consts(L)[0] if level else 1
    nch, nblk = (n + CHUNK - 1) // CHUNK, (n + bs - 1) // bs
    word = fill * 0x01010101
    a = {"prev": np.full(n, word, np.uint32), "cand": np.full(n * kw, word, np.uint32), "res": np.full(nch, word, np.uint32),
         "dst": np.full(nch, word * 0x100000001, np.uint64), "slots": np.full(nch * SLOT, fill, np.uint8), "out": np.full(out_cap(n), fill, np.uint8),
         "total": np.zeros(max(nblk, 1), np.uint64)}
    used = L.xl_stages(data, n, block_size, level, *(a[k].ctypes.data for k in ("prev", "cand", "res", "slots", "dst", "out")), out_cap(n),
                       a["total"].ctypes.data)
    assert 0 <= used <= out_cap(n)
    a["total"] = a["total"][:nblk]
    a["used"] = used
    return a


def price_table(L):
    t = np.zeros(128, np.uint16)
    L.xl_price_table(t.ctypes.data)
    return t


def corpora(size):
    """The three corpora of tools/deflate_corpora.py, `size` bytes each (its builders, not the script's own run, as
    tools/xz_bench.py takes them)."""
    import os
    origin = os.path.join(hostbuild.ROOT, "tools", "deflate_corpora.py")
    src = open(origin).read().split("depths = ")[0]
    g = {"__name__": "deflate_corpora_src", "__file__": origin}
    exec(compile(src, origin, "exec"), g)
    g["SIZE"] = size
    return {"text": g["text"](), "sources": g["fill"](g["sources"]()), "binaries": g["fill"](g["binaries"]())}
