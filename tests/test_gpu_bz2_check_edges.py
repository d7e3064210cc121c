"""The .bz2 self-check's four steps alone (snaphash_bz2_check_device) on the block tables of tests/bz2_check_cases.py: every
verdict -- status and offset -- must be the host model's bit for bit (tests/bz2_check_host_harness.cpp runs bz2_check_core.h on
the CPU, and tests/test_bz2_check_host.py holds that model against libbz2).  The compressed buffer and the staged buffer lie
between 4 KiB of canary that must come back untouched, their own bytes are read only, and the verdict array lies between
canary words.  All but three cases are level-1 pieces (at most 79 872 bytes); the three level-9 full blocks are a text block, a
periodic one and one that ends in a 259-byte run.  Tables of 1, 2 and 33 blocks with a refused block first, last and alone, and
one of 1 000 (four groups of the install side's batch).  Then the chain: Context.bzip2_buffer of every bz2enc_cases input, cut
at the scanned block starts and checked -- every block accepted -- and, after one bit inside one block's body is changed in the
HBM copy, exactly that block refused."""
import ctypes

import numpy as np
import pytest

import bz2_check_cases as C
import bz2enc_cases as E
from snappy_amd import Context, SnaphashError, _lib

pytestmark = [pytest.mark.gpu, pytest.mark.kernels_only("kernels on tables the test wrote: names FLAG_GPU_ONLY itself")]

CANARY = 4096
FILL = 0xA5
VFILL = 0xC3C3C3C3
VPAD = 16
EINVAL = -1


@pytest.fixture(scope="module")
def L():
    return C.load_harness()


@pytest.fixture(scope="module")
def kctx(built_lib):
    with Context(device=0, flags=_lib.FLAG_GPU_ONLY) as c:
        yield c


@pytest.fixture(scope="module")
def good(L):
    return C.good_cases(L, big=False)


def framed(data):
    """bytes -> a device tensor: canary, the bytes, canary"""
    import torch
    h = np.full(len(data) + 2 * CANARY, FILL, dtype=np.uint8)
    h[CANARY:CANARY + len(data)] = np.frombuffer(data, dtype=np.uint8)
    return torch.from_numpy(h).cuda()


def whole(t, data, what):
    h = t.cpu().numpy()
    assert (h[:CANARY] == FILL).all() and (h[CANARY + len(data):] == FILL).all(), "the canary around " + what
    assert bytes(h[CANARY:CANARY + len(data)]) == data, what + " itself was written"


def device_check(c, d_z, d_in, case):
    """snaphash_bz2_check_device itself, the verdicts between canary words: -> [(status, offset)]."""
    import torch
    torch.cuda.synchronize()
    nb = case.nb
    a64 = lambda t: (ctypes.c_uint64 * nb)(*t)
    v = (ctypes.c_uint32 * (2 * nb + 2 * VPAD))(*([VFILL] * (2 * nb + 2 * VPAD)))
    rc = _lib.lib().snaphash_bz2_check_device(c._h, d_z.data_ptr() + CANARY, len(case.z), a64(case.z_beg), a64(case.z_end), d_in.data_ptr() + CANARY,
                                              len(case.data), a64(case.in_off), a64(case.in_len), (ctypes.c_uint32 * nb)(*case.crc), case.level, nb,
                                              ctypes.addressof(v) + 4 * VPAD)
    assert rc == 0, _lib.lib().snaphash_last_error(c._h)
    assert all(x == VFILL for x in v[:VPAD]) and all(x == VFILL for x in v[VPAD + 2 * nb:]), "the canary around the verdicts"
    return [(v[VPAD + 2 * k], v[VPAD + 2 * k + 1]) for k in range(nb)]


def run_cases(kctx, L, cases):
    ins = {}
    for c in cases:
        if c.data not in ins:
            ins[c.data] = framed(c.data)
        d_in, d_z = ins[c.data], framed(c.z)
        want = C.host_verdicts(L, c)
        got = device_check(kctx, d_z, d_in, c)
        assert got == want, "%s: (the kernels', the host model's) %s" % (c.name, [x for x in zip(got, want) if x[0] != x[1]][:4])
        if c.expect is not None:
            assert [s for s, _ in got] == c.expect, c.name
        for k, off in c.offsets.items():
            assert got[k][1] == off, c.name
        whole(d_z, c.z, "d_z of " + c.name)
    for data, t in ins.items():
        whole(t, data, "d_in")


@pytest.mark.parametrize("which", ["model", "libbz2"])
def test_good_cases_match_the_host_model(kctx, L, good, which):
    cases = [c for c in good if c.name.startswith(which) and "periodic_ab1000" not in c.name]
    assert len(cases) > 100 and all(c.level == 1 and max(c.in_len) <= E.PIECE for c in cases)
    assert {"model_L1_rle_1", "model_L1_rle_64", "model_L1_rle_65", "model_L1_rle_65537", "model_L1_piece_exact", "model_L1_run_260_first",
            "model_L1_run_259_last", "model_L1_small[0]@1", "model_L1_periodic_u2_op+1", "model_L1_one_byte_piece",
            "model_L1_runs_of_four_piece"} <= {c.name for c in good}
    run_cases(kctx, L, cases)


def test_every_origptr_of_a_tie_group_in_one_table(kctx, L, good):
    """(ab)^1000 with each of its 1 000 origPtr values: one table of 1 000 blocks, four groups of the decoder's batch."""
    cases = [c for c in good if "periodic_ab1000" in c.name]
    assert len(cases) == 1000
    table = C.combine("ab1000", cases)
    d_z, d_in = framed(table.z), framed(table.data)
    got = device_check(kctx, d_z, d_in, table)
    assert got == [(C.OK, 2000)] * 1000 and got == C.host_verdicts(L, table)
    whole(d_z, table.z, "d_z")
    whole(d_in, table.data, "d_in")


def test_damaged_cases_match_the_host_model(kctx, L):
    cases = C.damaged_cases(L)
    assert len(cases) > 150
    seen = {C.OK}
    for c in cases:
        seen.update(c.expect or [])
    assert seen == set(range(9))
    run_cases(kctx, L, cases)


@pytest.mark.parametrize("which", ["text", "periodic", "run_259_last"])
def test_level9_full_blocks(kctx, L, which):
    P9 = E.piece(9)
    data = {"text": lambda: C.X.text(P9, seed=91), "periodic": lambda: C.no_runs(P9 // 8, 92) * 8,
            "run_259_last": lambda: C.X.text(P9 - 259, seed=93) + b"r" * 259}[which]()
    assert len(data) == P9
    good9 = C.libbz2_case(L, which, data, 9)  # (libbz2's sort: the host model's would take this test's budget on the periodic block)
    d = bytearray(data)
    d[-1] ^= 0x20
    cases = [good9, good9.with_("last_byte", "staged", [C.BYTE], {0: P9 - 1}, data=bytes(d)), good9.with_("short", "length", [C.LENGTH], {0: P9 - 1}, in_len=[P9 - 1])]
    run_cases(kctx, L, cases)


@pytest.mark.parametrize("nb", [1, 2, 33])
def test_small_tables_with_a_refused_block_first_last_and_alone(kctx, L, nb):
    blocks = [C.model_case(L, "t%d" % k, C.X.text(2000 + 37 * k, seed=300 + k), 1) for k in range(nb)]
    table = C.combine("table_%d" % nb, blocks)
    assert table.nb == nb
    d_z, d_in = framed(table.z), framed(table.data)
    got = device_check(kctx, d_z, d_in, table)
    assert got == C.host_verdicts(L, table) == [(C.OK, n) for n in table.in_len]
    for bad in sorted({0, nb - 1}):  # a staged byte of that block alone
        at = table.in_len[bad] // 3
        d = bytearray(table.data)
        d[table.in_off[bad] + at] ^= 0x40
        c = table.with_("bad_%d" % bad, "staged", None, data=bytes(d))
        d_bad = framed(c.data)
        got = device_check(kctx, d_z, d_bad, c)
        assert got == C.host_verdicts(L, c), bad
        assert [k for k, (s, _) in enumerate(got) if s != C.OK] == [bad] and got[bad] == (C.BYTE, at), (bad, got[bad])
        whole(d_bad, c.data, "d_in")
    whole(d_z, table.z, "d_z")
    whole(d_in, table.data, "d_in")


@pytest.mark.parametrize("name", [n for n, d in E.cases() if len(d)])
def test_chain_the_producers_output_is_accepted(kctx, L, name):
    import torch
    data = dict(E.cases())[name]
    z = kctx.bzip2_buffer(data, 1)
    case = C.stream_case(L, "chain_" + name, z, data, 1, E.PIECE)
    d_z, d_in = framed(z), framed(data)
    got = device_check(kctx, d_z, d_in, case)
    assert got == [(C.OK, n) for n in case.in_len], name
    # one bit inside one block's body, changed in the HBM copy from here: exactly that block is refused
    bad = case.nb // 2
    zb, ze = case.z_beg[bad], case.z_end[bad]
    hb = C.header_bits(z, zb)
    bit = zb + hb + (ze - zb - hb) // 2
    assert zb + hb <= bit < ze
    changed = case.with_("changed", "flip", None, z=C.flip_bit(z, bit))
    d_z[CANARY + bit // 8] = changed.z[bit // 8]
    torch.cuda.synchronize()
    got = device_check(kctx, d_z, d_in, changed)
    assert got == C.host_verdicts(L, changed), name
    assert [k for k, (s, _) in enumerate(got) if s != C.OK] == [bad], (name, got[bad])
    whole(d_in, data, "d_in")
    whole(d_z, changed.z, "d_z")


def test_refused_arguments(kctx):
    d = framed(b"abc")
    p = d.data_ptr() + CANARY

    def refused(*a):
        with pytest.raises(SnaphashError) as e:
            kctx.bz2_check_device(*a)
        assert e.value.code == EINVAL

    refused(p, 3, [0], [24], p, 3, [0], [3], [0], 0)    # a level outside 1..9
    refused(p, 3, [0], [24], p, 3, [0], [3], [0], 10)
    refused(0, 3, [0], [24], p, 3, [0], [3], [0], 9)    # null compressed bytes
    refused(p, 3, [0], [24], 0, 3, [0], [3], [0], 9)    # null staged stream
    assert kctx.bz2_check_device(p, 3, [], [], p, 3, [], [], [], 9) == []              # no block: nothing to do
    assert kctx.bz2_check_device(p, 3, [0], [24], p, 3, [0], [3], [0], 9) == [(C.BLOCK, 4)]  # ("abc" is no block magic)
    assert kctx.bz2_check_device(0, 0, [0], [1], 0, 0, [0], [0], [0], 9) == [(C.TABLE, 0)]   # (no bytes at all: the entry lies outside them)
    whole(d, b"abc", "the buffer")
