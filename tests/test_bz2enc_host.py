"""Writing data.tar.bz2 on the CPU: the host model of snappy_amd/csrc/bzip2_enc_core.h (the routines the GPU kernels run,
compiled for the host by tests/bz2enc_host_harness.cpp) over every input of tests/bz2enc_cases.py, at levels 1 and 9.
libbz2's verdict (Python's bz2) is the oracle; the project's own host decoder reads the same files through the unmodified
tests/bzip2_host_harness.cpp; the files are parsed again with bzip2_core.h's reader for what a decoder does not show (block
count, CRCs, code lengths, selector counts); the BWT stage is held against a naive sort of rotations; the size against
libbz2's on the same pieces; and a stand-alone program runs the model under ASan/UBSan.  The kernels that run the same
header are checked in tests/test_gpu_bz2enc.py.  For tests/test_gpu_bz2enc_edges.py, which holds every array the kernels
leave against the model's: the stage arrays of tests/bz2enc_stage_model.h (be_stages) chain to the model's file, equal plain
Python references of RLE1, the BWT and MTF on bz2enc_cases.edge_cases(), read back through bzip2_core.h's block decoder,
and every edge input is what its name says."""
import bz2
import ctypes
import functools
import glob
import itertools
import os
import random

import numpy as np
import pytest

import bz2enc_cases as B
import xz_cases as X
import hostbuild
from conftest import ROOT
from test_bzip2_host import bh, serial  # noqa: F401  (the decoder harness's fixture)

P = ctypes.POINTER
INFO = 8  # uint64 a block: be_encode's and be_parse's rows


@functools.lru_cache(maxsize=None)
def load_model():
    """tests/bz2enc_host_harness.cpp, loaded once a process with every prototype (it keeps no state between calls)."""
    L = hostbuild.shared("tests/bz2enc_host_harness.cpp")
    L.be_encode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, P(ctypes.c_size_t), P(ctypes.c_uint64), ctypes.c_size_t,
                            P(ctypes.c_size_t)]
    L.be_encode.restype = ctypes.c_void_p
    L.be_free.argtypes = [ctypes.c_void_p]
    L.be_piece.argtypes = [ctypes.c_uint32]
    L.be_piece.restype = ctypes.c_uint32
    L.be_ntables.argtypes = [ctypes.c_uint32]
    L.be_ntables.restype = ctypes.c_uint32
    L.be_rle1.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p]
    L.be_rle1.restype = ctypes.c_uint32
    L.be_bwt.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p]
    L.be_bwt.restype = ctypes.c_uint32
    L.be_mtf.argtypes = [ctypes.c_char_p, ctypes.c_uint32, P(ctypes.c_uint16), P(ctypes.c_uint32)]
    L.be_mtf.restype = ctypes.c_uint32
    L.be_code_lengths.argtypes = [P(ctypes.c_uint32), ctypes.c_uint32, ctypes.c_uint32, ctypes.c_char_p]
    L.be_code_lengths.restype = None
    L.be_parse.argtypes = [ctypes.c_char_p, ctypes.c_size_t, P(ctypes.c_uint64), ctypes.c_size_t, P(ctypes.c_uint32), P(ctypes.c_uint32),
                           P(ctypes.c_uint32)]
    L.be_parse.restype = ctypes.c_int64
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.be_slot_words.argtypes = L.be_rle_cap.argtypes = [u32]
    L.be_slot_words.restype = L.be_rle_cap.restype = u32
    L.be_stages.argtypes = [vp, vp, vp, u32, u32, u32, u32] + [vp] * 9 + [u64, vp]
    L.be_stages.restype = ctypes.c_int64
    L.be_stages_from_last.argtypes = [vp, vp, vp, u32, u32, u32, u32] + [vp] * 8 + [u64, vp]
    L.be_stages_from_last.restype = ctypes.c_int64
    L.be_read_slot.argtypes = [vp, u32, vp, u32, P(u32), P(u32), P(u32), P(u64)]
    L.be_read_slot.restype = ctypes.c_int32
    return L


def encode(L, data, level, cap=64):
    """-> (the model's stream, [rle_n, orig_ptr, nmtf, ntables, nsel, crc, bits, 0] a block)"""
    n, nb = ctypes.c_size_t(), ctypes.c_size_t()
    info = (ctypes.c_uint64 * (INFO * cap))()
    p = L.be_encode(data, len(data), level, ctypes.byref(n), info, cap, ctypes.byref(nb))
    z = ctypes.string_at(p, n.value)
    L.be_free(p)
    assert nb.value <= cap
    return z, [list(info[INFO * k:INFO * k + INFO]) for k in range(nb.value)]


def parse(L, z, cap=64):
    """-> (level, stored combined CRC, folded CRC, [bit, crc, orig_ptr, ntables, nsel, longest code, n, nused] a block)"""
    rows = (ctypes.c_uint64 * (INFO * cap))()
    level, comb, fold = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    k = L.be_parse(z, len(z), rows, cap, ctypes.byref(level), ctypes.byref(comb), ctypes.byref(fold))
    assert 0 <= k <= cap, k
    return level.value, comb.value, fold.value, [list(rows[INFO * i:INFO * i + INFO]) for i in range(k)]


def rle1(L, data):
    out = ctypes.create_string_buffer(len(data) // 4 * 5 + 8)
    n = L.be_rle1(data, len(data), out)
    return out.raw[:n]


def bwt(L, data):
    out = ctypes.create_string_buffer(max(len(data), 1))
    op = L.be_bwt(data, len(data), out)
    return out.raw[:len(data)], op


# ---- the stages' arrays (bz2enc_stage_model.h), as snaphash_bzenc_stages_device must leave them ----
FILL = 0xA5
MAP_BYTES, SEL_STRIDE, RES_WORDS = 516, 18048, 6
ARRAYS = (("rle", np.uint8), ("last", np.uint8), ("syms", np.uint16), ("maps", np.uint8), ("sel", np.uint8), ("slots", np.uint32),
          ("res", np.uint32), ("dst", np.uint64), ("out", np.uint32))
ZEROED = ("slots", "res", "out")  # the launchers memset them; every other array starts as the fill
GUARD_OUT_WORDS = 64              # d_out of a call that is to fail: not written at all


def edge_cap(L, e):
    return e.cap or L.be_rle_cap(e.level)


def stage_counts(L, nblk, cap, out_words):
    """elements of every array"""
    room = cap + 64
    return {"rle": nblk * room, "last": nblk * room, "syms": nblk * room, "maps": nblk * MAP_BYTES, "sel": nblk * SEL_STRIDE,
            "slots": nblk * L.be_slot_words(cap), "res": nblk * RES_WORDS, "dst": nblk, "out": out_words}


def put_columns(last, columns, cap):
    for k, (col, _, _) in enumerate(columns):
        last[k * (cap + 64):k * (cap + 64) + len(col)] = np.frombuffer(col, dtype=np.uint8)


def stages(L, e):
    """The model's arrays of one Edge -> {array name: numpy array, "total": bits (-1: a block is over), "over": a flag a
    block, "cap", "nblk"}; out is cut to the words the placed bits need (GUARD_OUT_WORDS of fill where nothing is placed)."""
    cap = edge_cap(L, e)
    nblk = len(e.columns if e.kind == "last" else e.ranges)
    cnt = stage_counts(L, nblk, cap, nblk * L.be_slot_words(cap) + 2)
    a = {k: (np.zeros(cnt[k], dtype=dt) if k in ZEROED else np.full(cnt[k] * np.dtype(dt).itemsize, FILL, dtype=np.uint8).view(dt)) for k, dt in ARRAYS}
    over = np.zeros(max(nblk, 1), dtype=np.uint8)
    ptr = {k: a[k].ctypes.data for k, _ in ARRAYS}
    if e.kind == "last":
        put_columns(a["last"], e.columns, cap)
        meta = [np.array([f(c) for c in e.columns], dtype=np.uint32) for f in (lambda c: len(c[0]), lambda c: c[1], lambda c: c[2])]
        total = L.be_stages_from_last(*(m.ctypes.data for m in meta), nblk, cap, e.carry, e.carry_bits,
                                      *(ptr[k] for k, _ in ARRAYS[1:]), cnt["out"], over.ctypes.data)
    else:
        offs = np.array([o for o, _ in e.ranges], dtype=np.uint64)
        lens = np.array([n for _, n in e.ranges], dtype=np.uint64)
        buf = np.frombuffer(e.data, dtype=np.uint8) if e.data else np.zeros(1, dtype=np.uint8)
        total = L.be_stages(buf.ctypes.data, offs.ctypes.data, lens.ctypes.data, nblk, cap, e.carry, e.carry_bits,
                            *(ptr[k] for k, _ in ARRAYS), cnt["out"], over.ctypes.data)
    if total < 0:
        a["dst"] = np.full(8 * nblk, FILL, dtype=np.uint8).view(np.uint64)
        a["out"] = np.full(4 * GUARD_OUT_WORDS, FILL, dtype=np.uint8).view(np.uint32)
    else:
        assert not a["out"][(total + 31) // 32:].any()
        a["out"] = a["out"][:max((total + 31) // 32, 1)].copy()
    a.update(total=total, over=over[:nblk], cap=cap, nblk=nblk)
    return a


def read_slot(L, slot, cap):
    """One slot's bits through the install side's decoder -> (status, last column, origPtr, CRC, the bit it ended at)"""
    out = np.zeros(cap + 64, dtype=np.uint8)
    n, op, crc, end = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
    slot = np.ascontiguousarray(slot)
    st = L.be_read_slot(slot.ctypes.data, len(slot), out.ctypes.data, len(out), ctypes.byref(n), ctypes.byref(op), ctypes.byref(crc), ctypes.byref(end))
    return st, out[:n.value].tobytes(), op.value, crc.value, end.value


def finish(level, out, total, crcs, carry_bits=0):
    """The host's part around the kernels' bits out[carry_bits .. total): "BZh" + level in front, the end-of-stream magic,
    the combined CRC and the padding behind."""
    raw = out.tobytes()
    v = int.from_bytes(raw, "big") >> (8 * len(raw) - total) if total else 0
    v &= (1 << (total - carry_bits)) - 1
    comb = 0
    for c in crcs:
        comb = ((comb << 1 | comb >> 31) & 0xffffffff) ^ int(c)
    v = (v << 48 | 0x177245385090) << 32 | comb
    bits = total - carry_bits + 80
    pad = -bits % 8
    return b"BZh" + bytes([48 + level]) + (v << pad).to_bytes((bits + pad) // 8, "big")


def pieces_edge(name, data, level):
    """`data` cut as the producer cuts it"""
    Pn = B.piece(level)
    return B.Edge(name, "pieces", level, 0, 0, 0, data, [(o, min(Pn, len(data) - o)) for o in range(0, len(data), Pn)], None)


# ---- plain references of the first three stages ----
def rle1_py(d):
    out = bytearray()
    for c, grp in itertools.groupby(d):
        run = len(list(grp))
        for part in [259] * (run // 259) + ([run % 259] if run % 259 else []):
            out += bytes([c]) * min(part, 4)
            if part >= 4:
                out.append(part - 4)
    return bytes(out)


def mtf_py(last):
    """-> (symbols: RUNA 0, RUNB 1, list position p as p + 1, the end-of-block symbol last; the used-byte count)"""
    lst, out, run = sorted(set(last)), [], 0

    def flush(run):
        while run:  # bijective base 2, least digit first
            out.append(0 if run & 1 else 1)
            run = (run - 1) // 2 if run & 1 else (run - 2) // 2
    for b in last:
        if lst[0] == b:
            run += 1
            continue
        flush(run)
        run = 0
        p = lst.index(b)
        lst.insert(0, lst.pop(p))
        out.append(p + 1)
    flush(run)
    return out + [len(set(last)) + 1], len(set(last))


def naive_bwt(b):
    """Sorted cyclic rotations, equal ones by start index: (last column, origPtr)."""
    n = len(b)
    d = b + b
    sa = sorted(range(n), key=lambda i: (d[i:i + n], i))
    return bytes(b[i - 1] for i in sa), sa.index(0)


@pytest.fixture(scope="module")
def be():
    return load_model()


def all_cases(be):
    def nmtf_of(d):
        return encode(be, d, 1)[1][0][2]
    return [(n, d, lv) for n, d in list(B.cases()) + B.nmtf_cases(nmtf_of) for lv in (1, 9)] + list(B.big_cases())


@pytest.fixture(scope="module")
def files(be):
    """(name, level) -> (data, the model's stream, its block infos), computed once and left alone."""
    return {(n, lv): (d,) + encode(be, d, lv) for n, d, lv in all_cases(be)}


def test_piece_sizes(be):
    assert [be.be_piece(lv) for lv in range(1, 10)] == [B.piece(lv) for lv in range(1, 10)]
    for lv in range(1, 10):
        assert B.piece(lv) % 512 == 0 and B.piece(lv) * 5 // 4 <= 100000 * lv - 19 < (B.piece(lv) + 512) * 5 // 4


def test_libbz2_reads_every_file(files):
    for (name, lv), (data, z, info) in files.items():
        assert bz2.decompress(z) == data, (name, lv)


def test_the_librarys_host_decoder_reads_every_file(files, bh):
    for (name, lv), (data, z, info) in files.items():
        rc, out = serial(bh, z)
        assert rc == 0 and out == data, (name, lv)


def test_the_files_parsed_again(files, be, bh):
    for (name, lv), (data, z, info) in files.items():
        level, comb, fold, rows = parse(be, z)
        Pn = B.piece(lv)
        assert level == lv and comb == fold, (name, lv)
        assert len(rows) == len(info) == (len(data) + Pn - 1) // Pn, (name, lv)
        for k, (row, bi) in enumerate(zip(rows, info)):
            piece = data[k * Pn:(k + 1) * Pn]
            assert row[1] == bi[5] == bh.bh_crc(piece, len(piece)), (name, lv, k)
            assert row[5] <= 17, (name, lv, k)                       # no code longer than 17 bits
            assert row[4] == bi[4] == (bi[2] + 49) // 50, (name, lv, k)  # selectors: ceil(nMTF / 50)
            assert row[3] == bi[3] == be.be_ntables(bi[2]), (name, lv, k)
            assert row[6] == bi[0] == len(rle1(be, piece)) and row[2] == bi[1], (name, lv, k)


def test_the_cases_are_what_their_names_say(files, be):
    f = {k: v for k, v in files.items()}
    Pn = B.PIECE
    for t in B.NMTF_LIMITS:
        assert f[("nmtf_%d" % t, 1)][2][0][2] == t
    assert [f[("nmtf_%d" % t, 1)][2][0][3] for t in B.NMTF_LIMITS] == [2, 3, 3, 4, 4, 5, 5, 6]
    one = f[("one_byte_3", 1)][2]
    assert len(one) == 1 and one[0][2:5] == [3, 2, 1] and parse(be, f[("one_byte_3", 1)][1])[3][0][7] == 1  # RUNA RUNA EOB; an alphabet of 3
    assert rle1(be, f[("one_byte_piece", 1)][0])[:10] == b"\0\0\0\0\xff" * 2 and f[("one_byte_piece", 1)][2][0][3:5] == [2, 1]
    assert f[("runs_of_four_piece", 1)][2][0][0] == Pn * 5 // 4 == 99840 <= 100000 - 19
    assert parse(be, f[("all_256_values", 1)][1])[3][0][7] == 256
    assert parse(be, f[("one_map_row", 1)][1])[3][0][7] == 16
    assert len(f[("six_pieces", 1)][2]) == 6
    # the runs: what RLE1 makes of them
    assert rle1(be, b"r" * 255) == b"rrrr" + bytes([251]) and rle1(be, b"r" * 259) == b"rrrr" + bytes([255])
    assert rle1(be, b"r" * 260) == b"rrrr" + bytes([255]) + b"r" and rle1(be, b"r" * 263) == b"rrrr" + bytes([255]) + b"rrrr" + bytes([0])
    assert rle1(be, b"r" * 518) == (b"rrrr" + bytes([255])) * 2
    for k in range(6):  # the run cut by the piece's end is two runs
        d = f[("run_across_%d" % k, 1)][0]
        want = b"\x07" * min(k, 4) + (bytes([k - 4]) if k >= 4 else b"")
        first = rle1(be, d[:Pn])
        assert d[Pn - k:Pn + 5 - k] == b"\x07" * 5 and d[Pn - k - 1] != 7 and first.endswith(want) and first[-len(want) - 1] != 7
    # zero runs of 2^k - 1, 2^k, 2^k + 1 in the MTF stream: ab x m has the last column b^m a^m
    for name, data in B.sorted_runs():
        last, op = bwt(be, data)
        m = len(data) // 2
        assert last == b"b" * m + b"a" * m and op == 0, name
    # a periodic block's origPtr: rotation 0 is the first of its tie group
    assert bwt(be, b"ab" * 1000) == (b"b" * 1000 + b"a" * 1000, 0)
    assert bwt(be, b"ba" * 7)[1] == 7


def test_bwt_against_a_naive_sort(be):
    r = random.Random(5)
    inputs = [b"a", b"ab", b"ba", b"aa", b"aaa", b"abab", b"abcabcabc", b"banana", b"\x00" * 64, b"ab" * 500, b"abc" * 333,
              bytes(range(256)), X.text(3000, seed=6), X.rnd(2500, seed=7), rle1(be, b"\x00" * 2590)]
    for n in (1, 2, 3, 63, 64, 65, 1023, 1024, 1025):
        inputs.append(bytes(r.randrange(3) for _ in range(n)))
    for d in inputs:
        assert bwt(be, d) == naive_bwt(d), d[:20]


def test_code_lengths_at_the_limit(be):
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    for freqs in (fib[:30], fib, [0] * 10 + fib[:28], [1] * 258, [0] * 258, [900000] + [0] * 257, [5, 0, 0]):
        arr = (ctypes.c_uint32 * len(freqs))(*freqs)
        out = ctypes.create_string_buffer(len(freqs))
        be.be_code_lengths(arr, len(freqs), 17, out)
        lens = list(out.raw)
        assert 1 <= min(lens) and max(lens) <= 17, freqs[:5]
        assert sum(2 ** (17 - l) for l in lens) == 2 ** 17, freqs[:5]  # a complete prefix code
    # the unlimited code of the Fibonacci frequencies is deeper than 17: the limit did something
    arr = (ctypes.c_uint32 * 30)(*fib[:30])
    out = ctypes.create_string_buffer(30)
    be.be_code_lengths(arr, 30, 40, out)
    assert max(out.raw) == 29


def corpus(kind, n):
    if kind == "text":
        return X.text(n, seed=77)
    if kind == "sources":
        paths = sorted(glob.glob(os.path.join(ROOT, "snappy_amd", "csrc", "*.*")) + glob.glob(os.path.join(ROOT, "tests", "*.py")))
        src = b"".join(open(p, "rb").read() for p in paths if p.endswith((".h", ".hip", ".cpp", ".inc", ".py")))
        return (src * (n // len(src) + 1))[:n] if len(src) < n else src[:n]
    so = open(os.path.join(ROOT, "snappy_amd", "libsnaphash.so"), "rb").read()  # (built_lib: it is there)
    assert len(so) >= n
    return so[:n]


@pytest.mark.parametrize("kind", ["text", "sources", "binaries"])
def test_size_against_libbz2_on_the_same_pieces(be, built_lib, kind):
    """The algorithm is libbz2's; what is left free is the length-limited code construction and the tie rules.  Measured
    (this test prints them): text 0.9998, sources 0.9999, binaries 0.9998 of libbz2's bytes."""
    data = corpus(kind, 3 * B.piece(9) // 2)
    z, info = encode(be, data, 9)
    assert bz2.decompress(z) == data
    Pn = B.piece(9)
    ref = sum(len(bz2.compress(data[o:o + Pn], 9)) for o in range(0, len(data), Pn))
    print("bz2enc size %s: model %d, libbz2 on the pieces %d, ratio %.4f" % (kind, len(z), ref, len(z) / ref))
    assert len(z) <= 1.01 * ref


def edges_of(be):
    """bz2enc_cases.edge_cases() with the model's nMTF (the search for group counts needs it)"""
    if not hasattr(be, "_nmtf_of"):
        be._nmtf_of = lambda d, level: encode(be, d, level)[1][0][2]
    return B.edge_cases(be._nmtf_of)


@pytest.fixture(scope="module")
def edge_models(be):
    """Edge name -> (the Edge, the model's arrays), computed once and left alone."""
    return {e.name: (e, stages(be, e)) for e in edges_of(be)}


def blocks_of(e, m):
    """(k, the block's input or None, rle_n, the arrays' views of block k)"""
    room, sw = m["cap"] + 64, len(m["slots"]) // max(m["nblk"], 1)
    for k in range(m["nblk"]):
        piece = e.data[e.ranges[k][0]:e.ranges[k][0] + e.ranges[k][1]] if e.kind != "last" else None
        res = [int(v) for v in m["res"][k * RES_WORDS:(k + 1) * RES_WORDS]]
        view = {"rle": m["rle"][k * room:(k + 1) * room], "last": m["last"][k * room:(k + 1) * room], "syms": m["syms"][k * room:(k + 1) * room],
                "maps": m["maps"][k * MAP_BYTES:(k + 1) * MAP_BYTES], "sel": m["sel"][k * SEL_STRIDE:(k + 1) * SEL_STRIDE],
                "slot": m["slots"][k * sw:(k + 1) * sw]}
        yield k, piece, res, view


def test_the_stage_arrays_chain_to_the_models_file(be, files):
    """"BZh1", be_stages' bits over the producer's pieces and the footer are be_encode's file, at level 1 for every input
    and at level 9 for those that are more than one block there."""
    for (name, lv), (data, z, info) in files.items():
        if not data or (lv == 9 and len(data) <= B.piece(9) and (name, 1) in files):
            continue
        e = pieces_edge(name, data, lv)
        m = stages(be, e)
        assert m["total"] == sum(bi[6] for bi in info) and not m["over"].any(), (name, lv)
        assert [int(v) for v in m["dst"]] == list(itertools.accumulate([0] + [bi[6] for bi in info[:-1]])), (name, lv)
        assert finish(lv, m["out"], m["total"], [bi[5] for bi in info]) == z, (name, lv)
        for k, piece, res, v in blocks_of(e, m):
            assert res == [info[k][0], info[k][1], info[k][2], info[k][6], 0, 0], (name, lv, k)


def test_plain_references_equal_the_stage_arrays(be, edge_models, bh):
    """RLE1, the BWT and MTF written out plainly in Python (the BWT by sorting rotations up to 3000 bytes, be_bwt -- held
    against that sort above -- beyond; MTF up to 120 000 symbols, or any length over few byte values) give every edge
    input's arrays, the fill behind each stage's length included; every slot reads back through the install side's
    decoder to the block's last column, origPtr and CRC; the bits placed are the slots' bits."""
    for name, (e, m) in edge_models.items():
        room = m["cap"] + 64
        for k, piece, res, v in blocks_of(e, m):
            rn, op, nmtf, bits, over = res[:5]
            if e.kind != "last":
                ref = rle1_py(piece)
                if m["over"][k]:
                    assert e.kind == "guard" and len(ref) > m["cap"] and rn == 0 and over == 1, (name, k)
                    # a pair that would end behind the room is dropped whole: its first byte's place keeps the fill
                    pair_at_end = len(ref) > room and piece_emits_pair_at(piece, room - 1)
                    stored = room - 1 if pair_at_end else min(room, len(ref))
                    assert v["rle"][:stored].tobytes() == ref[:stored] and (v["rle"][stored:] == FILL).all(), (name, k)
                    assert (v["last"] == FILL).all(), (name, k)
                    continue
                assert rn == len(ref) and v["rle"][:rn].tobytes() == ref and (v["rle"][rn:] == FILL).all(), (name, k)
                assert ref == rle1(be, piece) and bh.bh_crc(piece, len(piece)) == read_slot(be, v["slot"], m["cap"])[3], (name, k)
                assert (v["last"][:rn].tobytes(), op) == (naive_bwt(ref) if rn <= 3000 else bwt(be, ref)), (name, k)
            else:
                assert (m["rle"] == FILL).all() and (rn, op) == (len(e.columns[k][0]), e.columns[k][1]), (name, k)
                assert v["last"][:rn].tobytes() == e.columns[k][0], (name, k)
            assert over == 0 and (v["last"][rn:] == FILL).all(), (name, k)
            last = v["last"][:rn].tobytes()
            if rn <= 120000 or len(set(last)) <= 32:
                syms, nused = mtf_py(last)
                assert nmtf == len(syms) and v["syms"][:nmtf].tolist() == syms, (name, k)
                used = sorted(set(last))
                assert v["maps"][:256].tolist() == [int(c in used) for c in range(256)], (name, k)
                assert v["maps"][256:512].tolist() == [sum(u < c for u in used) & 255 for c in range(256)], (name, k)
                assert int(v["maps"][512:].view(np.uint32)[0]) == nused, (name, k)
            assert (v["syms"][nmtf:] == FILL * 0x101).all() and (v["sel"][(nmtf + 49) // 50:] == FILL).all(), (name, k)
            assert v["sel"][:(nmtf + 49) // 50].max() < be.be_ntables(nmtf), (name, k)
            st, col, op2, crc2, end = read_slot(be, v["slot"], m["cap"])
            assert (st, col, op2, end) == (0, last, op, bits) and not v["slot"][(bits + 31) // 32:].any(), (name, k)
            if e.kind == "last":
                assert crc2 == e.columns[k][2], (name, k)
        if m["total"] >= 0:  # the placement: block after block from carry_bits on, the carry's bits in front
            raw = int.from_bytes(m["out"].tobytes(), "big")
            nb = 32 * len(m["out"])
            assert len(m["out"]) == (m["total"] + 31) // 32 and raw >> (nb - e.carry_bits) == e.carry >> (8 - e.carry_bits), name
            at = e.carry_bits
            for k, piece, res, v in blocks_of(e, m):
                assert int(m["dst"][k]) == at, (name, k)
                sl = int.from_bytes(v["slot"].tobytes(), "big") >> (32 * len(v["slot"]) - res[3])
                assert raw >> (nb - at - res[3]) & ((1 << res[3]) - 1) == sl, (name, k)
                at += res[3]
            assert at == m["total"] and raw & ((1 << (nb - at)) - 1) == 0, name


def piece_emits_pair_at(piece, o):
    """Does RLE1 of `piece` put a fourth byte and its count at output offsets o, o + 1?"""
    out = 0
    for c, grp in itertools.groupby(piece):
        run = len(list(grp))
        for part in [259] * (run // 259) + ([run % 259] if run % 259 else []):
            if part >= 4 and out + 3 == o:
                return True
            out += min(part, 4) + (part >= 4)
    return False


def run_digits(syms):
    """the value of a RUNA / RUNB run, least digit first"""
    return sum((d + 1) << i for i, d in enumerate(syms))


def test_the_edge_inputs_are_what_their_names_say(be, edge_models):
    EE = b"\xee"
    assert list(edge_models) == B.edge_names()
    # RLE1: where the runs lie in the kernel's 1024-lane tiles, and what the model makes of them
    e, m = edge_models["rle1_tile_edges"]
    what = B.rle1_tile_edges()[1]
    assert len(what) == m["nblk"] and not m["over"].any()
    seen = set()
    for (k, piece, res, v), (kind, L, off) in zip(blocks_of(e, m), what):
        rle = v["rle"][:res[0]].tobytes()
        if kind == "run":
            assert piece[off:off + L] == EE * L and piece[off + L] != 0xee and (off == 0 or piece[off - 1] != 0xee)
            want = EE * 4 + bytes([min(L, 259) - 4]) + (EE * min(L - 259, 4) + (bytes([L - 263]) if L >= 263 else b"") if L > 259 else b"")
            assert rle[off:off + len(want)] == want and rle[off + len(want)] != 0xee, (L, off)
            seen.add((L, off % B.TILE))
        elif kind == "long_run":
            assert piece[off:off + L] == EE * L and off // B.TILE + 2 == (off + L - 1) // B.TILE  # it ends two tiles on
            assert rle[off:off + 9 * 5 + 4] == (EE * 4 + b"\xff") * 9 + EE * 4 and rle[off + 49] == L - 9 * 259 - 4
        elif kind == "cut_run":
            o, n = e.ranges[k]
            assert piece[-L:] == EE * L and piece[-L - 1] != 0xee and e.data[o + n:o + n + 300] == EE * 300
            assert rle.endswith(EE * min(L, 4) + (bytes([L - 4]) if L >= 4 else b"")) and res[0] == 1500 + min(L, 4) + (L >= 4)
        else:
            assert len(piece) == L
    assert seen == {(L, o % B.TILE) for L in B.RUN_LENS for o in B.RUN_OFFS} and {o % B.TILE for o in B.RUN_OFFS} == {0, 1019, 1020, 1021, 1022, 1023}
    assert sorted(L for kind, L, _ in what if kind == "len") == [1, 2, 1023, 1024, 1025]
    for lv, cap in ((1, 99840), (9, 899840)):  # RLE1's output is the cap to the byte
        e, m = edge_models["fours_full_piece_level%d" % lv]
        assert len(e.data) == B.piece(lv) and m["cap"] == cap and int(m["res"][0]) == cap and m["total"] > 0
    # MTF: the list positions, and the runs of the front byte against the 64-symbol tiles
    e, m = edge_models["mtf_positions"]
    what = B.mtf_edges()[1]
    for (k, _, res, v), w in zip(blocks_of(e, m), what):
        nused = int(v["maps"][512:].view(np.uint32)[0])
        if w[0] == "position":
            assert v["syms"][:res[2]].tolist() == [w[1] + 1] * 700 + [w[1] + 2] and nused == w[1] + 1
        elif w[0] == "sparse":
            used = np.flatnonzero(v["maps"][:256])
            assert 8 < nused == len(used) <= 200 and (v["maps"][256:512][used] != used).any()
        elif w[0] == "n":
            assert res[0] == w[1]
        else:
            assert nused == 1 and v["syms"][:res[2]].tolist()[-1] == 2 and run_digits(v["syms"][:res[2] - 1].tolist()) == 500
    assert [w[1] for w in what if w[0] == "position"] == list(B.MTF_POSITIONS) and [w[1] for w in what if w[0] == "n"] == [1, 63, 64, 65]
    e, m = edge_models["front_runs"]
    what = B.front_run_edges()[1]
    for (k, _, res, v), (R, start) in zip(blocks_of(e, m), what):
        syms = v["syms"][:res[2]].tolist()
        digits = list(itertools.takewhile(lambda s: s < 2, reversed(syms[:-1])))[::-1]
        assert run_digits(digits) == R and res[0] == start + R and start % 64 in (60, 61, 62, 63, 0) and start >= 64, (R, start)
    assert {R for R, _ in what} == set(B.FRONT_RUNS) >= {1, 2, 3, 63, 64, 65, 1023, 1024, 1025} and len(what) == 5 * len(B.FRONT_RUNS)
    # coding: the group counts at which a lane's share of groups steps, the last group's length, the most a block can have
    e1, m1 = edge_models["group_counts_level1"]
    nm = [int(m1["res"][k * RES_WORDS + 2]) for k in range(m1["nblk"])]
    assert tuple((n + 49) // 50 for n in nm[:5]) == B.GROUP_COUNTS_L1 and tuple((n - 1) % 50 + 1 for n in nm[5:]) == B.LAST_GROUPS
    e2, m2 = edge_models["group_counts_level2"]
    assert tuple((int(m2["res"][k * RES_WORDS + 2]) + 49) // 50 for k in range(m2["nblk"])) == B.GROUP_COUNTS_L2
    assert [-(-g // 1024) for g in B.GROUP_COUNTS_L1 + B.GROUP_COUNTS_L2] == [1, 1, 1, 1, 2, 2, 2, 3]
    words = [(int(m1["res"][k * RES_WORDS + 3]) + 31) // 32 for k in range(m1["nblk"])]  # concat: a sweep is 2048 words, 256 a workgroup
    assert min(words) < 256 and any(256 < w < 2048 for w in words) and max(words) > 2048
    e, m = edge_models["most_groups_level9"]
    assert int(m["res"][0]) == 899840 and int(m["res"][2]) == 899841 and (899841 + 49) // 50 == 17997 <= 18002
    freq = np.bincount(m["syms"][:899841], minlength=28).astype(np.uint32)
    assert len(freq) == 28 and freq[0] == freq[1] == 0
    lens = ctypes.create_string_buffer(28)
    be.be_code_lengths(freq.ctypes.data_as(P(ctypes.c_uint32)), 28, 40, lens)
    assert max(lens.raw) > 17  # without the limit the code is deeper than what is written
    e, m = edge_models["fibonacci_level9"]
    assert e.data == B.big_cases()[3][1] and m["nblk"] == 1
    # concat: every bit offset a block can start and end at, with bits held back in front
    for cb in (0, 1, 7):
        e, m = edge_models["concat_%d_blocks_carry_%d" % (B.CONCAT_BLOCKS, cb)]
        assert e.carry_bits == cb and (e.carry != 0) == (cb != 0) and all(1 <= n <= 200 for _, n in e.ranges) and int(m["dst"][0]) == cb
        ends = [int(m["dst"][k]) + int(m["res"][k * RES_WORDS + 3]) - 1 for k in range(m["nblk"])]
        assert {int(d) & 31 for d in m["dst"]} == set(range(32)) == {x & 31 for x in ends}, cb
    # the guards: exactly cap is taken; one block with more, and no more than 1000 bytes behind its cap + 64
    e, m = edge_models["guard_exactly_cap"]
    assert [int(m["res"][k * RES_WORDS]) for k in (1, 4)] == [B.GUARD_CAP] * 2 and not m["over"].any() and m["total"] > 0
    lens_seen = set()
    for name, (e, m) in edge_models.items():
        if e.kind != "guard":
            continue
        assert m["cap"] == B.GUARD_CAP and m["total"] == -1 and m["over"].tolist() == [int(k == (2 if name.endswith("last") else 1)) for k in range(m["nblk"])]
        k = m["over"].tolist().index(1)
        n = len(rle1_py(e.data[e.ranges[k][0]:e.ranges[k][0] + e.ranges[k][1]]))
        assert B.GUARD_CAP < n <= B.GUARD_CAP + 64 + 1000, name
        lens_seen.add(n)
        if name.endswith("middle"):
            assert e.ranges[k + 1][1] == 1 and m["nblk"] == k + 3
        else:
            assert k == m["nblk"] - 1
    assert lens_seen >= set(B.GUARD_OUTPUTS)
    e, m = edge_models["guard_straddle_last"]
    assert piece_emits_pair_at(e.data[e.ranges[2][0]:], B.GUARD_CAP + 63) and m["rle"][3 * (B.GUARD_CAP + 64) - 1] == FILL


def test_bz2enc_host_model_under_asan_and_ubsan(tmp_path, be):
    """Host code only, in a program of its own (tests/asan_bz2enc.cpp): the model over every input, each from a heap buffer
    of exactly its size, the stage model (be_stages' routines and the slot reader) over the edge inputs that run with a small
    cap, and 2000 random inputs of up to 200 KiB at random levels, decoded with bzip2_core.h."""
    exe = hostbuild.sanitized(["tests/asan_bz2enc.cpp"])
    args = ["2000", "1"]
    cases = [c for c in all_cases(be) if c[2] == 1 or len(c[1]) <= 3000 or c in B.big_cases()]
    for i, (name, data, lv) in enumerate(cases):
        p = tmp_path / ("c%03d" % i)
        p.write_bytes(data)
        args += [str(p), str(lv)]
    edges = [e for e in edges_of(be) if e.level == 1 and e.cap]  # the small ones: every array a heap buffer of exactly its size
    assert {"rle1_tile_edges", "mtf_positions", "front_runs", "guard_exactly_cap", "guard_straddle_middle"} <= {e.name for e in edges}
    for i, e in enumerate(edges):
        p, q = tmp_path / ("e%03d" % i), tmp_path / ("r%03d" % i)
        if e.kind == "last":
            p.write_bytes(b"".join(c for c, _, _ in e.columns))
            offs = [sum(len(c) for c, _, _ in e.columns[:k]) for k in range(len(e.columns))]
            q.write_text("".join("%d %d %d %d\n" % (o, len(c), op, crc) for o, (c, op, crc) in zip(offs, e.columns)))
        else:
            p.write_bytes(e.data)
            q.write_text("".join("%d %d\n" % r for r in e.ranges))
        args += ["-l" if e.kind == "last" else "-e", str(p), str(q), str(e.level), str(e.cap), str(e.carry), str(e.carry_bits)]
    out = hostbuild.run_sanitized(exe, args, timeout=900)
    assert out.stdout.split() == ["ok"] * (len(cases) + len(edges)) + ["random", "2000"]
