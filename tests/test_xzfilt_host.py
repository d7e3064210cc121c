"""The .xz filters PowerPC, IA64, SPARC and Delta on the CPU: snappy_amd/csrc/bcj_core.h and delta_core.h compiled for the
host (tests/xzfilt_host_harness.cpp) and held against liblzma through Python's lzma (tests/xzfilt_cases.py says how) -- the
filters in both directions on every edge input, the word filters' cut run stretch by stretch, Delta's three decode passes
and two encode passes modelled tile by tile and lane by lane at tiles of 8, 64 and 65 536 bytes against the serial bytes;
xz_plan's third mode over hand-built Block headers, every verdict lzma.decompress's, and the host decoder over what is
accepted, with the two old modes' refusals unchanged; the producer's host model with a chain; and the filters' cases under
ASan/UBSan in a program of its own.  The kernels that run the same headers are checked in tests/test_gpu_xzfilt_edges.py,
the entry points in tests/test_gpu_xz_chains.py."""
import ctypes
import functools
import lzma

import pytest

import xzfilt_cases as F
import hostbuild


@functools.lru_cache(maxsize=None)
def load_xzfilt():
    """tests/xzfilt_host_harness.cpp, loaded once a process with every prototype (it keeps no state between calls)."""
    L = hostbuild.shared("tests/xzfilt_host_harness.cpp")
    L.xf_block.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32]
    L.xf_cut.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int]
    L.xf_cut.restype = None
    L.xf_delta_tiles.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int]
    L.xf_delta_tiles.restype = None
    L.xf_alignment.argtypes = [ctypes.c_uint32]
    L.xf_alignment.restype = ctypes.c_uint32
    P = ctypes.POINTER
    L.xf_plan.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, P(ctypes.c_uint64), P(ctypes.c_uint32), P(ctypes.c_uint32), P(ctypes.c_uint32),
                          P(ctypes.c_uint32), ctypes.c_size_t, ctypes.c_char_p]
    L.xf_decode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint, ctypes.c_int, P(ctypes.c_size_t), P(ctypes.c_int)]
    L.xf_decode.restype = ctypes.c_void_p
    L.xf_encode.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32, P(ctypes.c_uint32), P(ctypes.c_size_t), P(ctypes.c_int)]
    L.xf_encode.restype = ctypes.c_void_p
    L.xf_free.argtypes = [ctypes.c_void_p]
    return L


@pytest.fixture(scope="module")
def xf():
    return load_xzfilt()


def block(L, filt, encode, data, start=0, dist=0):
    buf = ctypes.create_string_buffer(bytes(data), len(data))
    assert L.xf_block(filt, dist, int(encode), buf, len(data), start) == 0
    return buf.raw


def cut(L, filt, encode, data, start, stretch, order):
    buf = ctypes.create_string_buffer(bytes(data), len(data))
    L.xf_cut(filt, int(encode), buf, len(data), start, stretch, order)
    return buf.raw


def delta_tiles(L, encode, data, d, tile, order, lanes=256):
    buf = ctypes.create_string_buffer(bytes(data), len(data))
    L.xf_delta_tiles(int(encode), buf, len(data), d, tile, lanes, order)
    return buf.raw


@pytest.mark.parametrize("filt", F.WORD_FILTERS, ids=lambda f: F.NAMES[f])
def test_word_filters_are_liblzmas_in_both_directions(xf, filt):
    changed = 0
    for name, data, start in F.word_cases(filt):
        for enc in (True, False):
            want = F.oracle(filt, enc, data, start)
            assert block(xf, filt, enc, data, start) == want, (name, enc)
            changed += want != data
    assert changed > 30  # the cases are not ones the filters leave alone


@pytest.mark.parametrize("filt", F.WORD_FILTERS, ids=lambda f: F.NAMES[f])
def test_a_start_offset_changes_the_bytes_and_the_partial_unit_stays(xf, filt):
    """The inputs exercise what they are named for: positions enter the result, the Block's last whole unit is converted and
    a candidate that lacks its last byte is not; liblzma agrees on each."""
    d = F.code(filt, 5000, 1)
    assert block(xf, filt, True, d, 0) != block(xf, filt, True, d, 4096)
    cand = F.candidate(filt)
    whole = bytes(256) + cand
    assert block(xf, filt, True, whole) != whole and F.oracle(filt, True, whole) != whole
    assert block(xf, filt, True, whole[:-1]) == whole[:-1] == F.oracle(filt, True, whole[:-1])
    assert xf.xf_alignment(filt) == F.UNIT[filt]


@pytest.mark.parametrize("filt", F.WORD_FILTERS, ids=lambda f: F.NAMES[f])
def test_the_kernels_cut_gives_the_serial_bytes(xf, filt):
    """bcj_stretch_apply, what bcj_apply_kernel runs a lane a stretch, over every case with stretches of 16, 64 and 256 bytes
    (multiples of a bundle, cut from the Block's first byte), ascending and descending: liblzma's bytes."""
    for name, data, start in F.word_cases(filt):
        for enc in (True, False):
            want = F.oracle(filt, enc, data, start)
            for stretch in (16, 64, 256):
                for order in (0, 1):
                    assert cut(xf, filt, enc, data, start, stretch, order) == want, (name, enc, stretch, order)


def test_ia64_every_template_and_slot_is_exercised(xf):
    """The template table by its effect: bundles whose three slots are all candidates change in exactly the slots the
    template's mask names, for every one of the 32 templates."""
    import random
    table = [0] * 16 + [4, 4, 6, 6, 0, 0, 7, 7, 4, 4, 0, 0, 4, 4, 0, 0]
    r = random.Random(3)
    for t in range(32):
        b = F.ia64_bundle(r, t)
        got = block(xf, F.IA64, True, bytes(16) + b, 0)[16:]
        assert got == F.oracle(F.IA64, True, bytes(16) + b, 0)[16:]
        x, y = int.from_bytes(b, "little"), int.from_bytes(got, "little")
        for s in range(3):
            addr = ((1 << 20) - 1) << (5 + 41 * s + 13) | 1 << (5 + 41 * s + 36)
            assert ((x ^ y) & addr != 0) == bool(table[t] >> s & 1), (t, s)  # (position 16 adds 1 to the 20-bit field: it changes)


def test_delta_is_liblzmas_in_both_directions(xf):
    for name, data, d in F.delta_cases():
        for enc in (True, False):
            assert block(xf, F.DELTA, enc, data, 0, d) == F.oracle(F.DELTA, enc, data, d), (name, enc)


@pytest.mark.parametrize("tile", [8, 64, 65536])
def test_deltas_tiles_give_the_serial_bytes(xf, tile):
    """The kernels' passes from delta_core.h's pieces -- sums, carry, apply; tails, encode -- with tiles of 8, 64 and
    65 536 bytes, the tiles and the lanes in ascending and in descending order: liblzma's bytes.  At 8 and 64 bytes a
    distance is longer than a tile, every tile begins at another column, and a row group is a fraction of a row."""
    for name, data, d in F.delta_cases():
        if tile < 65536 and len(data) > 3 * F.TILE:
            data = data[:F.TILE + d + 1]  # (the small tiles make the many-tile case of any input)
        for enc in (True, False):
            want = F.oracle(F.DELTA, enc, data, d)
            for order in (0, 1):
                assert delta_tiles(xf, enc, data, d, tile, order) == want, (name, enc, tile, order)


def test_ones_would_show_a_lost_carry(xf):
    """What xzfilt_cases.py says of its all-0x01 inputs, by the numbers: with d = 3 and d = 255 a tile's column sums are not
    0 modulo 256, so the second tile's bytes depend on the first's carry; with d = 4 they are 0, and they would not."""
    for d, hides in ((3, False), (255, False), (1, True), (2, True), (4, True), (16, True), (256, True)):
        sums = [len(range(c, F.TILE, d)) % 256 for c in range(d)]  # a tile's column sums of all-0x01
        assert all(s == 0 for s in sums) == hides, d
        assert hides or len(set(sums)) > 1, d  # and they differ from column to column
    whole = F.oracle(F.DELTA, False, b"\x01" * (F.TILE + 300), 3)  # liblzma's byte i: the ones of its column up to i
    assert all(whole[i] == (i // 3 + 1) % 256 for i in range(F.TILE - 300, F.TILE + 300))


def test_fewer_lanes_than_a_row_group_needs(xf):
    """lanes / d row groups: with 256 lanes d = 255 leaves one lane idle and d = 3 leaves one; with 6 lanes and d = 4 two
    are idle, and one group walks every row."""
    data = F.rnd(1000, 9)
    for d, lanes in ((4, 6), (3, 7), (5, 5), (1, 3)):
        for enc in (True, False):
            assert delta_tiles(xf, enc, data, d, 64, 0, lanes) == F.oracle(F.DELTA, enc, data, d), (d, lanes, enc)


# ---- the container: xz_plan's third mode and the host decoder ------------------------------------------------------------------

EINVAL, EFORMAT = -1, -9
PLAN_OK, PLAN_FORMAT, PLAN_UNSUPPORTED = 0, 1, 2
NONE, BCJ, ANY = 0, 1, 2  # kXzChainNone / Bcj / Any


def plan(L, z, mode):
    """-> (verdict, [(ids and params of a Block's chain, its bcj field)], text)"""
    n = ctypes.c_uint64()
    cap = 16
    nf, bcj = (ctypes.c_uint32 * cap)(), (ctypes.c_uint32 * cap)()
    ids, params = (ctypes.c_uint32 * (3 * cap))(), (ctypes.c_uint32 * (3 * cap))()
    why = ctypes.create_string_buffer(128)
    rc = L.xf_plan(z, len(z), mode, ctypes.byref(n), nf, ids, params, bcj, cap, why)
    blocks = [([(ids[3 * i + k], params[3 * i + k]) for k in range(nf[i])], bcj[i]) for i in range(min(n.value, cap))]
    return rc, blocks, why.value.decode()


def decode(L, z, mode, threads=4):
    n, rc = ctypes.c_size_t(), ctypes.c_int()
    p = L.xf_decode(z, len(z), threads, mode, ctypes.byref(n), ctypes.byref(rc))
    b = ctypes.string_at(p, n.value)
    L.xf_free(p)
    return rc.value, b


def test_every_chain_gets_liblzmas_verdict(xf):
    """Hand-built Block headers -- every permutation of one, two and three pre-filters drawn from all seven, four
    pre-filters, Delta properties of 0 and 2 bytes, each BCJ offset off its alignment and on it, LZMA2 not last, ids liblzma
    does not know -- through xz_plan in the new mode: accepted exactly where lzma.decompress accepts, and what is accepted
    decodes to lzma's bytes on 1 and 4 host threads."""
    files = F.chain_files()
    assert sum(p is None for _, _, p in files) >= 20 and sum(p is not None for _, _, p in files) >= 7 + 49 + 343
    for name, z, plain in files:
        rc, blocks, why = plan(xf, z, ANY)
        assert (rc == PLAN_OK) == (plain is not None), (name, rc, why)
        for t in (1, 4):
            got = decode(xf, z, ANY, t)
            assert got == (0, plain) if plain is not None else got[0] in (EINVAL, EFORMAT) and got[1] == b"", (name, t)
    by = {n: (z, p) for n, z, p in files}
    for name in ("ia64_offset_8", "powerpc_offset_2", "delta_props_0_bytes", "delta_props_2_bytes", "bcj_props_5_bytes"):  # properties: the file is bad
        assert by[name][1] is None and plan(xf, by[name][0], ANY)[0] == PLAN_FORMAT, name
    assert by["sparc_offset_4"][1] is not None
    for name, text in (("arm64_0x0a", "xz: unsupported filter 0x0A"), ("riscv_0x0b_behind_delta", "xz: unsupported filter 0x0B"),
                       ("three_pre_filters_no_lzma2", "xz: unsupported filter 0x04")):  # ids: handed back, the first such filter named
        rc, _, why = plan(xf, by[name][0], ANY)
        assert (rc, why) == (PLAN_UNSUPPORTED, text), name


def test_plan_hands_out_the_chain_as_the_header_names_it(xf):
    by = {n: z for n, z, _ in F.chain_files()}
    assert plan(xf, by["chain_delta_x86_powerpc"], ANY)[1] == [([(3, 3), (4, 0), (5, 4096)], 0)]
    assert plan(xf, by["chain_ia64_ia64"], ANY)[1] == [([(6, 16), (6, 16)], 0)]
    assert plan(xf, by["chain_armthumb"], ANY)[1] == [([(8, 2)], 8)]  # a chain of one of the old three: bcj says so, as before
    assert plan(xf, by["chain_armthumb"], BCJ)[1] == [([(8, 2)], 8)]
    assert plan(xf, by["chain_sparc"], ANY)[1] == [([(9, 4)], 0)]
    assert plan(xf, by["delta_dist_256"], ANY)[1] == [([(3, 256)], 0)]
    rc, blocks, _ = plan(xf, by["mixed_blocks_check_4"], ANY)
    assert rc == PLAN_OK and [b[0] for b in blocks] == [[(3, 2)], [(5, 0)], [], [(6, 0), (6, 0)], [(3, 3), (4, 0), (9, 0)], [(6, 32), (3, 256), (8, 6)]]
    assert len(plan(xf, by["two_streams"], ANY)[1]) == 4


def test_without_the_mode_the_old_refusals_stand(xf):
    """kXzChainNone and kXzChainBcj: what they answered before, text included -- the first filter that is not LZMA2 is named."""
    import bcj_cases as B
    for name, z, plain in F.chain_files():
        if not name.startswith("chain_"):
            continue
        first = {v: k for k, v in F.NAMES.items()}[name.split("_")[1]]
        text = "xz: unsupported filter 0x%02X" % first
        assert plan(xf, z, NONE)[::2] == (PLAN_UNSUPPORTED, text), name
        assert decode(xf, z, NONE) == (EINVAL, b""), name
        if name.count("_") == 1 and first in B.FILTERS:
            assert plan(xf, z, BCJ)[0] == PLAN_OK and decode(xf, z, BCJ) == (0, plain), name
        else:
            assert plan(xf, z, BCJ)[::2] == (PLAN_UNSUPPORTED, text), name
    for name, z, text in B.other_chain_files():  # the files the BCJ suite pins, in the two old modes
        for mode in (NONE, BCJ):
            assert plan(xf, z, mode)[::2] == (PLAN_UNSUPPORTED, text), (name, mode)
    for name, z, plain in B.good_files():  # and everything SNAPHASH_UNXZ_BCJ accepts, the new mode accepts
        assert decode(xf, z, ANY) == (0, plain), name
    for name, z in B.refused_files():
        assert plan(xf, z, ANY)[0] == PLAN_FORMAT, name
    assert decode(xf, B.check_over_filtered_file(), ANY) == (EFORMAT, b"")


def test_liblzmas_own_files_decode(xf):
    data = F.mixed(150000, 21)
    for chain in F.PRODUCER_CHAINS + ([F.SPARC, (F.DELTA, 255), F.POWERPC], [(F.IA64, 4096)]):
        z = F.liblzma_chain_file(data, chain)
        for t in (1, 4):
            assert decode(xf, z, ANY, t) == (0, data), (chain, t)
        assert decode(xf, z, NONE)[0] == EINVAL


# ---- the producer's host model ------------------------------------------------------------------------------------------------

def encode(L, data, block_size, chain):
    """chain: [id or (id, param)] -> (rc, the model's .xz file)"""
    words = [(f[0] | f[1] << 8) if isinstance(f, tuple) else f for f in chain]
    n, rc = ctypes.c_size_t(), ctypes.c_int()
    p = L.xf_encode(data, len(data), block_size, len(words), (ctypes.c_uint32 * max(len(words), 3))(*words[:3]), ctypes.byref(n), ctypes.byref(rc))
    b = ctypes.string_at(p, n.value)
    L.xf_free(p)
    return rc.value, b


def header_filters(z):
    """(the number of filters, the bytes of the filter entries in front of LZMA2's) of the first Block header of a file"""
    h = z[12:12 + (z[12] + 1) * 4]
    at = 2
    for bit in (0x40, 0x80):  # the sizes, where the header states them
        if h[1] & bit:
            while h[at] & 0x80:
                at += 1
            at += 1
    return (h[1] & 3) + 1, h[at:h.index(b"\x21\x01", at)]


@pytest.mark.parametrize("chain", F.PRODUCER_CHAINS, ids=lambda c: "_".join(F.NAMES[f[0] if isinstance(f, tuple) else f] for f in c))
def test_host_model_with_a_chain(xf, chain):
    """liblzma reads the model's file back, the library's own decoder does in the new mode and refuses without it, and the
    Block header names the chain with liblzma's bytes."""
    data = F.mixed(3 * 65536 + 1234, 77)
    theirs = header_filters(F.liblzma_chain_file(data[:1000], chain))
    for bs in (65536, 131072):
        rc, z = encode(xf, data, bs, chain)
        assert rc == 0
        assert lzma.decompress(z) == data
        assert decode(xf, z, ANY) == (0, data)
        assert decode(xf, z, NONE)[0] == EINVAL
        assert header_filters(z) == theirs and len(theirs[1]) == sum(3 if isinstance(f, tuple) else 2 for f in chain)
        rc, blocks, _ = plan(xf, z, ANY)
        assert [b[0] for b in blocks] == [[f if isinstance(f, tuple) else (f, 0) for f in chain]] * -(-len(data) // bs)
    assert encode(xf, b"", 65536, chain) == encode(xf, b"", 65536, [])  # no Block, no chain


def test_host_model_chain_of_one_is_the_filter(xf):
    """chain = [x86] writes byte for byte what filter = x86 writes (the BCJ suite's harness); and the refusals."""
    import test_bcj_host as T
    data = F.mixed(70000, 5)
    for f in (4, 7, 8):
        assert encode(xf, data, 65536, [f]) == T.encode(T.load_bcj(), data, 65536, f)
    assert encode(xf, data, 65536, []) == T.encode(T.load_bcj(), data, 65536, 0)
    for bad in ([3, 4, 5, 6], [(3, 0)], [(3, 257)], [2], [10], [0x21], [(4, 1)], [(9, 4)], [4, 0]):
        assert encode(xf, data[:100], 65536, bad) == (-1, b""), bad


def test_delta_helps_on_a_sample_ramp(xf):
    """What Delta is for: 16-bit samples that climb compress better behind delta:2 (the host model's sizes)."""
    ramp = b"".join(((i * 37) & 0xFFFF).to_bytes(2, "little") for i in range(1 << 16))
    assert len(encode(xf, ramp, 1 << 17, [(F.DELTA, 2)])[1]) < len(encode(xf, ramp, 1 << 17, [])[1]) // 4


def test_same_cases_under_asan_ubsan(tmp_path):
    """Host code only, in a program of its own (tests/asan_xzfilt.cpp): every case from a heap buffer of exactly its size."""
    exe = hostbuild.sanitized(["tests/asan_xzfilt.cpp"])
    cases = F.all_word_cases() + [(F.DELTA, name, data, d) for name, data, d in F.delta_cases()]
    args = []
    for i, (filt, name, data, param) in enumerate(cases):
        p = tmp_path / ("c%03d" % i)
        p.write_bytes(data)
        args += [str(p), str(filt), str(param)]
    out = hostbuild.run_sanitized(exe, args)
    assert out.stdout.split() == ["ok"] * len(cases)
