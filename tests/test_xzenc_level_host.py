"""The .xz writer's level on the CPU (snappy_amd/csrc/xz_enc_core.h): the host model of level 1 --
xzenc_find_set, the price tables and xzenc_chunk_priced, the very function the kernel runs, with its lanes emulated by a
loop -- through tests/xzenc_level_host_harness.cpp.  liblzma (Python's lzma) and the project's own host decoder read every
file back; level 0 through the new path is the plain model's file; the chunk's and the window's edges; the tie-break of
the relaxation with the lanes in both orders; the price table against -16 log2(p / 2048); the size against level 0 on the
three corpora; and a stand-alone program under ASan/UBSan.  The kernel is held against the same model in
tests/test_gpu_xzenc_level.py."""
import ctypes
import lzma
import math

import numpy as np
import pytest

import hostbuild
import xz_cases as X
import xzenc_cases as E
import xzenc_level_cases as V
from test_xz_host import load_xh

# offsets into the probability array (xz_core.h)
P_IS_MATCH, P_IS_REP, P_IS_REP_G0, P_IS_REP0_LONG, P_POS_SLOT, P_SPEC_POS, P_ALIGN, P_LEN, P_REP_LEN, LIT_BASE = 0, 192, 204, 240, 432, 688, 802, 818, 1332, 1846
LEN_CHOICE, LEN_CHOICE2, LEN_LOW, LEN_MID, LEN_HIGH = 0, 1, 2, 130, 258
N_PROBS = LIT_BASE + (0x300 << 3)
SLOTS = 44


@pytest.fixture(scope="module")
def xl():
    return V.load_level()


@pytest.fixture(scope="module")
def xh():
    return load_xh()


@pytest.fixture(scope="module")
def files(xl):
    """name -> (level-1 file, input, block size): every case through the host model once."""
    out = {}
    for name, data, bs in V.all_cases():
        rc, z = V.encode(xl, data, bs, 1)
        assert rc == 0, name
        out[name] = (z, data, bs)
    return out


def own_decode(L, z):
    n, rc = ctypes.c_size_t(), ctypes.c_int()
    p = L.xh_decode(z, len(z), 2, ctypes.byref(n), ctypes.byref(rc))
    b = ctypes.string_at(p, n.value)
    L.xh_free(p)
    return rc.value, b


def test_the_constants_are_the_ones_written_down(xl):
    assert V.consts(xl) == (4, 1024, 32, 256)


def test_liblzma_and_the_projects_decoder_read_every_level_1_file_back(files, xh):
    assert len(files) >= 2 * (len(E.cases()) - 1) + 15
    for name, (z, data, _) in files.items():
        assert lzma.decompress(z) == data, name
        assert own_decode(xh, z) == (0, data), name


def test_level_0_through_the_new_path_is_the_plain_models_file(xl):
    for name, data, bs in V.all_cases():
        if len(data) > 1 << 20 and name != "far_dists":
            continue
        assert V.encode(xl, data, bs, 0) == V.encode_plain(xl, data, bs), name
    assert V.encode(xl, b"abc", 65536, 2) == (-1, b"")  # no such level


def test_the_bytes_do_not_depend_on_the_order_of_the_lanes(xl, files):
    for name, (z, data, bs) in files.items():
        if len(data) <= 3 * E.B:
            assert V.encode(xl, data, bs, 1, descending=True) == (0, z), name


def test_no_operation_crosses_a_chunks_end_and_every_byte_is_coded(xl):
    for name, data, bs in V.edge_cases():
        s, res, _ = V.ops(xl, data, bs, 1)
        assert s[V.T_CROSSES] == 0, name
        assert s[V.T_MAX_DIST] < bs, name
        if V.STORED not in res:
            assert s[V.T_CODED] == len(data), name


def test_chunks_of_one_two_and_three_bytes(xl, files):
    for k in (1, 2, 3):
        z, data, bs = files["chunk_of_%d" % k]
        _, res, _ = V.ops(xl, data, bs, 1)
        assert len(res) == 2 and res[0] != V.STORED and res[1] == V.STORED, k  # (no LZMA chunk is smaller than its 6 + 5 bytes)


def test_a_run_is_cut_at_the_chunks_end(xl, files):
    _, data, bs = files["run_over_chunk_end"]
    s, res, rows = V.ops(xl, data, bs, 1, log=True)
    assert s[V.T_CROSSES] == 0 and V.STORED not in res
    ends = [int(r[1] + r[3]) for r in rows if r[0] in (V.OP_REP, V.OP_MATCH)]
    assert V.CHUNK in ends  # an operation ends exactly there: the run's 100 bytes in chunk 0 are not coded as literals


def test_full_windows_cut_matches_at_the_windows_end(xl, files):
    """In `full_windows` the paths never come together, so a window closes only when it is full, W positions behind its
    start: operations end at multiples of W from the chunk's start far more often than chance has it."""
    _, data, bs = files["full_windows"]
    w = V.consts(xl)[1]
    _, res, rows = V.ops(xl, data, bs, 1, log=True)
    assert V.STORED not in res
    pos, ends = 0, set()
    for kind, at, _, ln in rows:  # (literals carry no position: count along)
        assert kind == V.OP_LIT or at == pos
        pos += int(ln)
        ends.add(pos)
    assert pos == len(data)
    # (a window that closes early shifts the ones behind it off the multiples of W, until the next chunk starts at one; an
    # operation ends at a given position by chance once in a mean operation's length)
    full = [k * w for k in range(1, V.CHUNK // w) if k * w in ends]
    chance = (V.CHUNK // w) * len(rows) / len(data)
    assert w in full and len(full) >= 16 and len(full) >= 3 * chance, (full, chance)
    # and the candidates: several a position
    st = V.stages(xl, data, bs, 1)
    k = V.consts(xl)[0]
    cand = st["cand"].reshape(-1, k)
    assert (cand[:, k - 1] != 0).sum() >= 100 and (cand[V.CHUNK:, 1] != 0).mean() > 0.2  # several a position, K at some
    lens = cand >> 22
    filled = cand != 0
    assert ((lens[:, 1:] > lens[:, :-1]) | ~filled[:, 1:]).all()  # lengths strictly rising, 0 behind the last
    assert (filled[:, :-1] | ~filled[:, 1:]).all()
    d = (cand & 0x3FFFFF) + 1
    assert ((d[:, 1:] > d[:, :-1]) | ~filled[:, 1:]).all()        # a longer match is a farther one: the nearest of each length


def test_a_maximal_match_closes_the_window_and_is_taken_whole(xl, files):
    _, data, bs = files["zeros_273"]
    _, res, rows = V.ops(xl, data, bs, 1, log=True)
    assert V.STORED not in res
    long_ops = [(int(k), int(a), int(d), int(ln)) for k, a, d, ln in rows if ln == 273]
    assert len(long_ops) >= 4
    assert all(k == V.OP_REP or d == 1 for k, _, d, _ in long_ops)  # zeros: distance 1, as a match once and then as rep0
    # the position after a maximal match: the next operation starts right behind it
    pos = 0
    for kind, at, _, ln in rows:
        assert kind == V.OP_LIT or at == pos
        pos += int(ln)
    assert pos == len(data)


def test_periods_are_coded_by_rep0(xl, files):
    for p in (7, 300):
        _, data, bs = files["period_%d" % p]
        s, res, _ = V.ops(xl, data, bs, 1)
        assert all(r < 700 for r in res), (p, res)
        assert s[V.T_REP] >= 200 and s[V.T_MATCH] <= 4, (p, s)  # rep0 at 273 bytes over and over; a match a chunk to set it


def test_no_rep_in_front_of_the_blocks_first_byte(xl, files):
    _, data, bs = files["first_position"]
    _, _, rows = V.ops(xl, data, bs, 1, log=True)
    assert rows[0][0] == V.OP_LIT and rows[1][0] == V.OP_LIT  # 'a', 'b': nothing to copy from yet
    assert any(r[0] == V.OP_MATCH and r[2] == 2 for r in rows[:4])  # then the period of 2


def test_far_dists_with_k_candidates(xl, files):
    z, data, bs = files["far_dists"]
    s, res, rows = V.ops(xl, data, bs, 1, log=True)
    assert s[V.T_MAX_DIST] == E.FAR_MAX and V.STORED not in res
    dists = {int(r[2]) for r in rows if r[0] == V.OP_MATCH}
    assert set(E.FAR_DISTS) <= dists
    st = V.stages(xl, data, bs, 1)
    k = V.consts(xl)[0]
    assert int(st["cand"].reshape(-1, k)[E.FAR_MAX].max()) == (273 << 22 | (E.FAR_MAX - 1))


def test_hash_twins_are_no_candidates(xl, files):
    _, data, bs = files["hash_twins"]
    k = V.consts(xl)[0]
    cand = V.stages(xl, data, bs, 1)["cand"].reshape(-1, k)
    a1, b1, a2, b2 = E.TWIN_AT
    for ta, tb in ((a1, b1), (a2, b2)):
        assert all(c == 0 or tb - ((int(c) & 0x3FFFFF) + 1) != ta for c in cand[tb])
    assert int(cand[a2][0]) == (4 << 22 | (a2 - a1 - 1)) and not cand[a2][1:].any()


def test_incompressible_bytes_are_stored_at_both_levels(xl, files):
    _, data, bs = files["incompressible"]
    for level in (0, 1):
        _, res, _ = V.ops(xl, data, bs, level)
        assert res == [V.STORED] * 3, level


def test_the_stored_lzma_line(xl, files):
    """Around the line the result is LZMA iff 6 + csize < 3 + usize, and the coder gives up inside its loop once that can no
    longer hold: S_CODED tells which of the two places stored a chunk.  Level 1 crosses the line once, later than level 0
    or at the same k."""
    seen = []
    for k in V.MARGIN_KS:
        _, data, bs = files["margin_%d" % k]
        s, res, _ = V.ops(xl, data, bs, 1)
        assert len(res) == 1
        if res[0] != V.STORED:
            assert 6 + res[0] < 3 + V.CHUNK and s[V.T_CODED] == V.CHUNK, k
        seen.append((res[0] == V.STORED, s[V.T_CODED] < V.CHUNK))
        _, res0, _ = V.ops(xl, data, bs, 0)
        assert res0[0] == V.STORED or res[0] != V.STORED, k  # what level 0 still compresses, level 1 does too
    stored = [a for a, _ in seen]
    assert stored == sorted(stored) and not stored[0] and stored[-1]  # crossed once
    assert seen[-1][1]  # the give-up inside the loop did occur


# ---- the tie-break --------------------------------------------------------------------------------------------------------


def _tie_block():
    """'abcd' at 10, at 17 and at 34 = p, each followed by a byte of its own; everything else differs pairwise."""
    blk = bytearray(range(100, 160))
    for at, nxt in ((10, 1), (17, 2), (34, 3)):
        blk[at:at + 5] = b"abcd" + bytes([nxt])
    return bytes(blk), 34


def test_of_two_candidates_of_equal_price_the_lower_edge_index_wins(xl):
    """Two candidates of one length at distances 17 and 24: one distance slot (8), whose three more bits are priced from
    untouched probabilities -- equal prices.  The candidate in the lower slot of the position wins, whichever distance it
    holds, with the lanes in either order."""
    blk, p = _tie_block()
    k = V.consts(xl)[0]
    for first, second in ((17, 24), (24, 17)):
        cand = np.zeros((len(blk), k), np.uint32)
        cand[p][0] = 4 << 22 | (first - 1)
        cand[p][1] = 4 << 22 | (second - 1)
        for desc in (False, True):
            r, rows = V.chunk(xl, blk, cand, descending=desc)
            matches = [tuple(int(v) for v in row) for row in rows if row[0] == V.OP_MATCH]
            assert matches == [(V.OP_MATCH, p, first, 4)], (first, desc, matches)
            assert len(rows) == len(blk) - 3


def test_of_a_rep_and_a_match_of_equal_price_the_rep_wins(xl):
    """A run of 'a' from position 1 on: at position 2, rep0 (distance 1, the reset state's) and a candidate of distance 1
    copy the same eight bytes.  With every probability at its reset value the rep costs 7 bits and the match 11; the
    probabilities of IsRepG0 and IsRep0Long are set so that the two bits of rep0 cost 96 units where they cost 32:
    equal prices.  The rep has the lower edge index."""
    t = V.price_table(xl)
    # IsRepG0 far towards 0: rep1-3, which are distance 1 too after a reset, pay its dear side.  IsRep weighs a rep against
    # a match, IsRep0Long is rep0's alone.
    found = next(((i, j, q) for i in range(120, 128) for j in range(1, 40) for q in range(1, 127)
                  if int(t[i]) + int(t[j]) + int(t[127 - q]) - int(t[q]) == 96 and int(t[127 - i]) + 16 > int(t[i]) + int(t[j])
                  and int(t[127 - q]) + int(t[i]) + int(t[127 - j]) > int(t[q]) + 32 + 16), None)  # (a short rep and a rep of 7 is dearer)
    assert found is not None
    i, j, q = found
    blk = b"Q" + b"a" * 9 + bytes(range(200, 230))
    p, state, ps = 2, 0, 2
    probs = np.full(N_PROBS, 1024, np.uint16)
    probs[P_IS_REP_G0 + state] = 16 * i + 8                          # bit 0 is priced at t[i], bit 1 at t[127 - i]
    probs[P_IS_REP0_LONG + (state << 4) + ps] = 2048 - (16 * j + 8)  # bit 1 at t[j]
    probs[P_IS_REP + state] = 16 * q + 8                             # bit 0 at t[q], bit 1 at t[127 - q]
    rep = int(t[64]) + int(t[127 - q]) + int(t[i]) + int(t[j]) + 4 * int(t[64])   # IsMatch, IsRep; G0, Rep0Long; the length's four bits
    match = int(t[64]) + int(t[q]) + 4 * int(t[64]) + 6 * int(t[64])               # IsMatch, IsRep; the length; slot 0
    rep1 = int(t[64]) + int(t[127 - q]) + int(t[127 - i]) + int(t[64]) + 4 * int(t[64])
    assert rep == match < rep1
    k = V.consts(xl)[0]
    cand = np.zeros((len(blk), k), np.uint32)
    cand[p][0] = 8 << 22 | 0
    for desc in (False, True):
        r, rows = V.chunk(xl, blk, cand, probs=probs, descending=desc)
        assert [tuple(int(v) for v in row) for row in rows[:3]] == [(V.OP_LIT, 0xFFFFFFFF, 0, 1), (V.OP_LIT, 0xFFFFFFFF, 0, 1), (V.OP_REP, p, 0, 8)], (desc, rows[:4])
    probs[P_IS_REP0_LONG + (state << 4) + ps] = 2048 - (16 * (j - 1) + 8)  # the rep a little dearer: the match is taken
    r, rows = V.chunk(xl, blk, cand, probs=probs)
    assert tuple(int(v) for v in rows[2]) == (V.OP_MATCH, p, 1, 8)


def test_an_earlier_node_keeps_a_target_against_an_equal_price_from_a_later_node(xl):
    """'abcdefgh' twice: the candidate of eight bytes at p, and the one of seven at p + 1 behind a literal, reach the same
    node; the first is far cheaper.  And the find routine's candidates are what the chain holds, nearest first."""
    blk = bytes(range(50, 70)) + b"abcdefgh" + bytes(range(70, 80)) + b"abcdefgh" + bytes(range(80, 90))
    p = 38
    out = (ctypes.c_uint32 * 4)()
    xl.xl_find_set(blk, len(blk), p, len(blk), out)
    assert list(out) == [8 << 22 | 17, 0, 0, 0]
    k = V.consts(xl)[0]
    cand = np.zeros((len(blk), k), np.uint32)
    for q in range(p, p + 5):
        xl.xl_find_set(blk, len(blk), q, len(blk), out)
        cand[q] = list(out)
    _, rows = V.chunk(xl, blk, cand)
    assert [tuple(int(v) for v in r) for r in rows if r[0] == V.OP_MATCH] == [(V.OP_MATCH, p, 18, 8)]


def test_find_set_keeps_the_longest_k_of_rising_lengths(xl):
    """Six copies of a pattern, each agreeing with the last one byte further than the one after it: nearest first the
    chain offers lengths 4, 5, 6, 7, 8, 9, of which the longest four stay; all are cut at the chunk's end."""
    pat = b"0123456789"
    parts = []
    for keep in (9, 8, 7, 6, 5, 4):  # farthest first
        parts.append(pat[:keep] + bytes([200 + keep]) * 3)
    blk = b"".join(parts) + pat + b"!!!!"
    p = len(blk) - 14
    out = (ctypes.c_uint32 * 4)()
    xl.xl_find_set(blk, len(blk), p, len(blk), out)
    assert [c >> 22 for c in out] == [6, 7, 8, 9]
    dist = [(c & 0x3FFFFF) + 1 for c in out]
    assert dist == sorted(dist) and all(blk[p - d:p - d + (c >> 22)] == blk[p:p + (c >> 22)] for c, d in zip(out, dist))
    xl.xl_find_set(blk, len(blk), p, p + 7, out)  # the chunk ends seven bytes on
    assert [c >> 22 for c in out] == [4, 5, 6, 7]  # (the walk stops at the first candidate that reaches the chunk's end)
    xl.xl_find_set(blk, len(blk), p, p + 1, out)
    assert list(out) == [0, 0, 0, 0]


# ---- prices -----------------------------------------------------------------------------------------------------------------


def test_the_price_table_is_minus_16_log2(xl):
    t = V.price_table(xl)
    for i in range(128):
        want = -16 * math.log2((16 * i + 8) / 2048)
        assert abs(int(t[i]) - want) <= 1, (i, int(t[i]), want)
    assert int(t[64]) == 16 and int(t[127]) == 0 and (np.diff(t.astype(int)) <= 0).all()


def _bit(t, prob, bit):
    return int(t[((2048 - prob) if bit else prob) >> 4])


def _tree(t, probs, base, bits, value, rev=False):
    m, total = 1, 0
    for i in (range(bits) if rev else range(bits - 1, -1, -1)):
        b = (value >> i) & 1
        total += _bit(t, int(probs[base + m]), b)
        m = m << 1 | b
    return total


def test_length_slot_align_distance_and_literal_prices_are_the_sums_of_their_bits(xl):
    t = V.price_table(xl)
    r = np.random.default_rng(27)
    probs = r.integers(31, 2018, N_PROBS).astype(np.uint16)  # what an adaptive probability can be
    lenp, slotp, alignp = np.zeros(2 * 4 * 272, np.uint16), np.zeros(4 * SLOTS, np.uint16), np.zeros(16, np.uint16)
    dists = np.array([1, 2, 4, 5, 6, 7, 8, 17, 24, 96, 127, 128, 129, 1000, 65536, 1 << 20, (4 << 20) - 273], np.uint32)
    distp = np.zeros((len(dists), 8), np.uint32)
    litp = np.zeros(2, np.uint32)
    lit = bytes([0x5A, 0xC3])
    xl.xl_tables(probs.ctypes.data, lenp.ctypes.data, slotp.ctypes.data, alignp.ctypes.data, dists.ctypes.data, len(dists), distp.ctypes.data, lit,
                 litp.ctypes.data)
    lenp = lenp.reshape(2, 4, 272)
    for which, base in ((0, P_LEN), (1, P_REP_LEN)):
        for ps in range(4):
            for ln in (2, 3, 9, 10, 11, 17, 18, 19, 100, 272, 273):
                l = ln - 2
                if l < 8:
                    want = _bit(t, int(probs[base + LEN_CHOICE]), 0) + _tree(t, probs, base + LEN_LOW + (ps << 3), 3, l)
                elif l < 16:
                    want = _bit(t, int(probs[base + LEN_CHOICE]), 1) + _bit(t, int(probs[base + LEN_CHOICE2]), 0) + _tree(t, probs, base + LEN_MID + (ps << 3), 3, l - 8)
                else:
                    want = _bit(t, int(probs[base + LEN_CHOICE]), 1) + _bit(t, int(probs[base + LEN_CHOICE2]), 1) + _tree(t, probs, base + LEN_HIGH, 8, l - 16)
                assert int(lenp[which, ps, l]) == want, (which, ps, ln)
    slotp = slotp.reshape(4, SLOTS)
    for ls in range(4):
        for slot in range(SLOTS):
            assert int(slotp[ls, slot]) == _tree(t, probs, P_POS_SLOT + (ls << 6), 6, slot), (ls, slot)
    for v in range(16):
        assert int(alignp[v]) == _tree(t, probs, P_ALIGN, 4, v, rev=True), v
    for di, d in enumerate(dists):
        d1 = int(d) - 1
        slot = d1 if d1 < 4 else 2 * (d1.bit_length() - 1) + ((d1 >> (d1.bit_length() - 2)) & 1)
        for ln in range(2, 10):
            want = int(slotp[min(ln - 2, 3), slot])
            if slot >= 4:
                nb = (slot >> 1) - 1
                base = (2 | (slot & 1)) << nb
                if slot < 14:
                    want += _tree(t, probs, P_SPEC_POS + base - slot - 1, nb, d1 - base, rev=True)
                else:
                    want += 16 * (nb - 4) + int(alignp[(d1 - base) & 15])
            assert int(distp[di, ln - 2]) == want, (int(d), ln)
    # a literal behind 0x5A: plain in state 0; in state 7 against the match byte (rep0 = 0: the byte in front, 0x5A)
    lp = LIT_BASE + 0x300 * (0x5A >> 5)
    assert int(litp[0]) == _tree(t, probs, lp, 8, 0xC3)
    mb, offs, sym, want = 0x5A, 0x100, 1, 0
    for i in range(7, -1, -1):
        mb <<= 1
        mbit, bit = mb & offs, (0xC3 >> i) & 1
        want += _bit(t, int(probs[lp + offs + mbit + sym]), bit)
        sym = sym << 1 | bit
        offs &= mbit if bit else ~mbit
    assert int(litp[1]) == want


# ---- size: a condition --------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("block_size", [65536, 262144])
def test_level_1_is_strictly_smaller_than_level_0_on_the_three_corpora(xl, block_size):
    for name, data in V.corpora(256 * V.KiB).items():
        assert len(data) == 256 * V.KiB
        rc0, z0 = V.encode(xl, data, block_size, 0)
        rc1, z1 = V.encode(xl, data, block_size, 1)
        assert rc0 == 0 and rc1 == 0 and lzma.decompress(z1) == data
        print("%s in Blocks of %d: level 0 %d bytes, level 1 %d bytes (%+.2f %%)" % (name, block_size, len(z0), len(z1), 100.0 * (len(z1) - len(z0)) / len(z0)))
        assert len(z1) < len(z0), name


# ---- sanitizers: a program of its own ---------------------------------------------------------------------------------------


def test_the_level_under_asan_and_ubsan(tmp_path):
    """Host code only, in a program of its own (tests/asan_xzenc_level.cpp): the model at level 1 over every edge case and
    the smaller inputs of xzenc_cases, each from a heap buffer of exactly its size, and the host decoder over what it wrote."""
    exe = hostbuild.sanitized(["tests/asan_xzenc_level.cpp"])
    args, n = [], 0
    for i, (name, data, bs) in enumerate(V.all_cases()):
        if name.endswith("@128k") and len(data) > V.CHUNK:
            continue  # (the 64 KiB Blocks of the same input are in)
        p = tmp_path / ("c%03d" % i)
        p.write_bytes(data)
        args += [str(p), str(bs)]
        n += 1
    out = hostbuild.run_sanitized(exe, args)
    assert out.stdout.split() == ["ok"] * n
