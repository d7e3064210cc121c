"""The .bz2 producer's self-check on the CPU: snappy_amd/csrc/bz2_check_core.h's host model bz2_check_block, which the kernels
must agree with bit for bit, through tests/bz2_check_host_harness.cpp, against libbz2, on the tables of tests/bz2_check_cases.py.

Three things are asked.  Every GOOD case -- the producer's host model over every bz2enc_cases input at levels 1 and 9, libbz2's
own block for each piece, blocks at every bit alignment, the RLE1 chunk edges, runs at a piece's ends, periodic blocks with
every origPtr of their tie group -- is accepted, block by block, with offset in_len.  Every damaged case is refused with the
status (and, where the case states one, the offset) it was made for.  And for EVERY block of EVERY case, damaged or not, the
safety property: if the check accepts it, libbz2 decodes a stream of the block's stretch alone to exactly the piece.  A bit flip
the check accepts must therefore be one libbz2 decodes to the same bytes; how many there were is printed, not asserted."""
import ctypes
import struct

import pytest

import bz2_check_cases as C
import hostbuild


@pytest.fixture(scope="module")
def L():
    return C.load_harness()


@pytest.fixture(scope="module")
def good(L):
    return C.good_cases(L)


@pytest.fixture(scope="module")
def damaged(L):
    return C.damaged_cases(L)


@pytest.fixture(scope="module")
def verdicts(L, good, damaged):
    """The host model's verdicts, once for every case."""
    return {id(c): C.host_verdicts(L, c) for c in good + damaged}


def test_every_good_case_is_accepted(good, verdicts):
    names = {c.name for c in good}
    assert {"model_L1_six_pieces", "model_L9_six_pieces", "libbz2_L1_text_300k_p3", "model_L1_rle_65537", "libbz2_L1_rle_64", "model_L1_piece_exact",
            "model_L1_run_259_first", "libbz2_L1_run_260_last", "model_L1_small[0]@7", "libbz2_L1_small[0]@3", "model_L1_two_blocks[1]@5",
            "model_L1_periodic_u2_op+1", "model_L1_periodic_ab1000_op+999", "model_L1_one_byte_piece"} <= names
    for c in good:
        want = [(C.OK, n) for n in c.in_len]
        assert verdicts[id(c)] == want, (c.name, [x for x in zip(range(c.nb), verdicts[id(c)], want) if x[1] != x[2]][:4])


def test_damaged_cases_are_refused_with_their_status(damaged, verdicts):
    kinds = {c.kind for c in damaged}
    assert kinds == {"flip", "staged", "length", "crc", "end", "block", "origptr", "origptr_other", "cap", "table"}
    seen = {C.OK}
    for c in damaged:
        if c.expect is None:
            continue
        v = verdicts[id(c)]
        assert [s for s, _ in v] == c.expect, (c.name, v)
        for k, off in c.offsets.items():
            assert v[k][1] == off, (c.name, v)
        seen.update(c.expect)
    assert seen == set(range(9)), seen  # every status of the table occurs


def test_accepted_blocks_decode_to_their_bytes(good, damaged, verdicts):
    """The safety property, for every block of every case."""
    accepted_flips = refused_flips = blocks = 0
    for c in good + damaged:
        for k, (s, _) in enumerate(verdicts[id(c)]):
            blocks += 1
            if s == C.OK:
                assert C.block_ok(c, k), (c.name, k)
            if c.kind == "flip":
                accepted_flips += s == C.OK
                refused_flips += s != C.OK
    print("%d blocks; bit flips: %d accepted (each decodes to the staged bytes), %d refused" % (blocks, accepted_flips, refused_flips))
    assert accepted_flips + refused_flips == sum(1 for c in damaged if c.kind == "flip") >= C.HEAD_BITS + 16 + 32


def test_good_cases_are_good_by_libbz2(good):
    """The cases themselves: libbz2 decodes every good block's stretch to its piece (so an accepting check is not vacuous)."""
    for c in good:
        for k in range(c.nb):
            assert C.block_ok(c, k), (c.name, k)


def test_error_text(L):
    buf = ctypes.create_string_buffer(512)
    n = L.bc_error_text(b"data.tar.bz2", 12, 1, 12 * 719872 + 17, buf, 512)
    want = b"self-check: data.tar.bz2: block 12 does not decode to the bytes it was made from (status 1) at offset 8638481 of the tar stream"
    assert buf.value == want and n == len(want)
    L.bc_error_text(b"", 0, 8, 0, buf, 512)
    assert buf.value == b"self-check: : block 0 does not decode to the bytes it was made from (status 8) at offset 0 of the tar stream"
    n = L.bc_error_text(b"the buffer", (1 << 44) + 2, 7, (1 << 60) + 3, buf, 16)  # (cut to the room there is)
    assert buf.value == b"self-check: the" and n > 100


def test_stretches_come_from_the_scan(L):
    """stream_case's table: blocks back to back from bit 32, the last one ending at the end-of-stream magic."""
    c = C.model_case(L, "t", C.X.text(2 * C.E.PIECE + 10, 500), 1)
    assert c.nb == 3 and c.z_beg[0] == 32 and c.z_end[0] == c.z_beg[1] and c.z_end[1] == c.z_beg[2]
    assert C.get_bits(c.z, c.z_end[2], 48) == C.EOS_MAGIC and all(C.get_bits(c.z, b, 48) == C.BLOCK_MAGIC for b in c.z_beg)
    assert c.in_len == [C.E.PIECE, C.E.PIECE, 10] and c.in_off == [0, C.E.PIECE, 2 * C.E.PIECE]


def test_model_under_asan_and_ubsan(good, damaged, verdicts, tmp_path):
    """Host code only, in a program of its own (tests/asan_bz2_check.cpp): every case, each buffer on the heap at exactly its
    size, then with the buffers cut short and the tables shifted.  Its first pass's verdicts are the harness's."""
    exe = hostbuild.sanitized(["tests/asan_bz2_check.cpp"])
    cases = good + damaged
    inputs = tmp_path / "cases.bin"
    with open(inputs, "wb") as f:
        for c in cases:
            f.write(struct.pack("<QQQQ", len(c.z), len(c.data), c.nb, c.level) + c.z + c.data)
            for t in (c.z_beg, c.z_end, c.in_off, c.in_len, c.crc):
                f.write(struct.pack("<%dQ" % c.nb, *t))
    out_file = tmp_path / "verdicts.bin"
    out = hostbuild.run_sanitized(exe, [inputs, out_file], timeout=1800)
    print(out.stdout[-400:])
    assert out.stdout.startswith("%d cases, " % len(cases))
    want = b"".join(struct.pack("<II", *x) for c in cases for x in verdicts[id(c)])
    assert out_file.read_bytes() == want
