"""The .xz producer's self-check on the CPU: snappy_amd/csrc/lzma2_check_core.h, the walk lzma2_check_kernel runs, through
tests/lzma2_check_host_harness.cpp, against liblzma, on the chunk tables of tests/lzma2_check_cases.py.

Three things are asked.  Every GOOD case -- the producer's host model over every xzenc_cases input, liblzma's own chunks,
hand-coded ones -- is accepted, chunk by chunk.  Every damaged case of the staged-byte, table, end-byte, distance, length,
control, properties and header kinds is refused with the status (and, where the case states one, the offset) it was made
for, and its other chunks are accepted.  And for EVERY Block of EVERY case, damaged or not, the safety property: if the
walker accepts all its chunks, liblzma decodes the concatenated stretches as raw LZMA2 to exactly the Block's staged bytes
and reports the end.  A bit flip the walker accepts must therefore be one liblzma decodes to the same bytes; how many
there were is printed."""
import ctypes
import struct

import pytest

import lzma2_check_cases as C
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


def test_every_good_case_is_accepted(L, good):
    names = {c.name for c in good}
    assert {"model_far_dists", "model_incompressible", "liblzma_p9_text_text_rnd", "dist_is_front", "rep3_first", "short_rep_first",
            "matched_literal_prev_chunk", "len273_ends_full_chunk", "one_byte_lzma", "blocks_64k"} <= names
    for c in good:
        v = C.host_verdicts(L, c)
        want = [(C.OK, min(C.CHUNK, len(c.data) - i * C.CHUNK)) for i in range(c.nch)]  # accepted: the walk came to the chunk's end
        assert v == want, (c.name, [x for x in zip(range(c.nch), v, want) if x[1] != x[2]][:4])


def test_damaged_cases_are_refused_with_their_status(L, damaged):
    kinds = {c.kind for c in damaged}
    assert kinds == {"flip", "staged", "table", "end_byte", "distance", "length", "control", "props", "header"}
    seen = set()
    for c in damaged:
        if c.expect is None:
            continue
        v = C.host_verdicts(L, c)
        assert [s for s, _ in v] == c.expect, (c.name, v)
        for i, off in getattr(c, "offsets", {}).items():
            assert v[i][1] == off, (c.name, v)
        seen.update(c.expect)
    assert seen == set(range(9)), seen  # every status of the table occurs


def test_accepted_blocks_decode_to_their_bytes(L, good, damaged):
    """The safety property, for every Block of every case."""
    accepted_flips = refused_flips = blocks = 0
    for c in good + damaged:
        v = C.host_verdicts(L, c)
        all_ok = True
        for k, (c0, cn, _) in enumerate(c.blocks()):
            ok = all(s == C.OK for s, _ in v[c0:c0 + cn])
            all_ok &= ok
            blocks += 1
            if ok:
                assert C.block_ok(c, k), (c.name, k, v[c0:c0 + cn])
        if c.kind == "flip":
            accepted_flips += all_ok
            refused_flips += not all_ok
    print("%d blocks; bit flips: %d accepted (each decodes to the staged bytes), %d refused" % (blocks, accepted_flips, refused_flips))
    assert accepted_flips + refused_flips == 88 + 24 + 8


def test_bit_flips_cover_every_header_and_start_bit(damaged):
    flips = {c.name for c in damaged if c.kind == "flip"}
    assert {"flip_%d_%02x" % (i, 1 << b) for i in range(11) for b in range(8)} <= flips


def test_error_text(L):
    buf = ctypes.create_string_buffer(512)
    n = L.lc_error_text(b"data.tar.xz", 3, 50, 2, 50 * 65536 + 17, buf, 512)
    want = (b"self-check: data.tar.xz: Block 3, chunk 50 does not decode to the bytes it was made from (status 2) at offset 3276817 "
            b"of the tar stream")
    assert buf.value == want and n == len(want)
    n = L.lc_error_text(b"", 0, 0, 8, 0, buf, 512)
    assert buf.value == b"self-check: : Block 0, chunk 0 does not decode to the bytes it was made from (status 8) at offset 0 of the tar stream"
    n = L.lc_error_text(b"the buffer", (1 << 40) + 1, (1 << 44) + 2, 7, (1 << 60) + 3, buf, 16)  # (cut to the room there is)
    assert buf.value == b"self-check: the" and n > 100


def test_stretch_ends_come_from_the_layout(L):
    """lc_encode's z_end is the next chunk's place, or the Block's data end: never read from the chunk's own header."""
    c = C.model_case(L, "t", C.X.text(3 * C.CHUNK + 10, 500), C.B)
    assert c.nch == 4
    assert c.z_end[0] == c.z_beg[1] and c.z_end[2] == c.z_beg[3]           # inside a Block: back to back
    assert c.z_end[1] < c.z_beg[2] and c.z[c.z_end[1] - 1] == 0             # a Block's last: behind its end byte; then the next Block's header
    assert c.z[c.z_end[3] - 1] == 0 and c.z_end[3] <= len(c.z)
    assert c.z_beg[2] - c.z_end[1] >= 8 + 12 and c.z[c.z_end[1] + 4] == C.FILL  # padding, Check and header: the host's, not written here


def test_walker_under_asan_and_ubsan(L, good, damaged, tmp_path):
    """Host code only, in a program of its own (tests/asan_lzma2_check.cpp): every case, each buffer on the heap at exactly
    its size, then with the buffers cut short and the tables shifted.  Its first pass's verdicts are the harness's."""
    exe = hostbuild.sanitized(["tests/asan_lzma2_check.cpp"])
    cases = good + damaged
    inputs = tmp_path / "streams.bin"
    with open(inputs, "wb") as f:
        for c in cases:
            f.write(struct.pack("<QQQQ", len(c.data), len(c.z), c.nch, c.bs) + c.data + c.z + struct.pack("<%dQ" % c.nch, *c.z_beg) +
                    struct.pack("<%dQ" % c.nch, *c.z_end))
    verdicts = tmp_path / "verdicts.bin"
    out = hostbuild.run_sanitized(exe, [inputs, verdicts], timeout=900)
    print(out.stdout[-400:])
    assert out.stdout.startswith("%d streams, " % len(cases))
    got = verdicts.read_bytes()
    want = b"".join(struct.pack("<II", *x) for c in cases for x in C.host_verdicts(L, c))
    assert got == want
