"""The build side's host-only parts on the CPU, through tests/snapbuild_host_harness.cpp.

The ar writer (snappy_amd/csrc/snap_core.h): what it writes is read back by ar_parse member for member, and held against a
few-line parser written here -- field widths, decimal and octal fields, the one padding byte.

The self-check's walker (snappy_amd/csrc/deflate_check_core.h, the code deflate_check_kernel runs) against zlib, on the
streams of tests/deflate_check_streams.py.  Two things are asked: every UNDAMAGED stream is accepted, chunk by chunk; and
for EVERY chunk of EVERY case, damaged or not, the safety property: if the walker accepts, zlib decodes the same stretch
(the 32 KiB in front as its dictionary, a final empty stored block behind it) to exactly the chunk and ends there.
Refusing a damaged stretch that zlib happens to decode to the same bytes is allowed.

RFC 1951 has no code for a distance of 32 769 (code 29 ends at 24 577 + 8 191 = 32 768), so no stream can carry "the same
match one byte farther": the bound min(32 768, bytes in front) is held at 32 769 on the walker's own test
(df_check_distance_ok) and, in streams, at its other arm -- distance 32 768 with 32 767 bytes in front is refused, with
32 768 in front accepted -- and at distance 4 with 3 in front."""
import ctypes
import functools
import struct

import pytest

import deflate_check_streams as S
import hostbuild

EINVAL = -1

HAND = S.hand_built()
VALID = S.valid_cases()
DAMAGED = S.damaged_cases()


@functools.lru_cache(maxsize=None)
def load_sb():
    """tests/snapbuild_host_harness.cpp, loaded once a process with every prototype (it keeps no state between calls)."""
    L = hostbuild.shared("tests/snapbuild_host_harness.cpp")
    u64p = ctypes.POINTER(ctypes.c_uint64)
    L.sb_ar_write.argtypes = [ctypes.c_char_p, u64p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int64, ctypes.c_uint32, ctypes.c_char_p,
                              ctypes.c_size_t, u64p]
    L.sb_ar_parse.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t]
    L.sb_deflate_check.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p, u64p, ctypes.c_uint32, ctypes.c_int,
                                   ctypes.POINTER(ctypes.c_uint32)]
    L.sb_deflate_check.restype = None
    L.sb_distance_ok.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    return L


@pytest.fixture(scope="module")
def sb():
    return load_sb()


# ---- the ar writer ----------------------------------------------------------------------------------------------------

def ar_write(L, members, mtime=1445212800, mode=0o100644):
    names = b"".join(n + b"\0" for n, _ in members)
    sizes = (ctypes.c_uint64 * max(1, len(members)))(*[len(d) for _, d in members])
    data = b"".join(d for _, d in members)
    cap = 8 + sum(61 + len(d) for _, d in members) + 16
    out = ctypes.create_string_buffer(cap)
    n = ctypes.c_uint64()
    rc = L.sb_ar_write(names, sizes, len(members), data, mtime, mode, out, cap, ctypes.byref(n))
    return rc, out.raw[:n.value]


def ar_parse(L, blob):
    text = ctypes.create_string_buffer(1 << 16)
    rc = L.sb_ar_parse(blob, len(blob), text, len(text))
    mem = []
    for line in text.value.decode().splitlines():
        h, off, size = line.split("\t")
        mem.append((bytes.fromhex(h), int(off), int(size)))
    return rc, mem


def plain_ar(blob):
    """the container as ar(5) states it, restated in a few lines: -> [(name, mtime, uid, gid, mode, data)]"""
    assert blob[:8] == b"!<arch>\n"
    at, out = 8, []
    while at < len(blob):
        h = blob[at:at + 60]
        assert len(h) == 60 and h[58:60] == b"`\n"
        name, mtime, uid, gid, mode, size = h[0:16], h[16:28], h[28:34], h[34:40], h[40:48], h[48:58]
        for f in (mtime, uid, gid, mode, size):  # digits, then spaces to the field's width
            assert f.rstrip(b" ").isdigit() and b" " not in f.rstrip(b" "), f
        n = int(size)
        data = blob[at + 60:at + 60 + n]
        assert len(data) == n
        at += 60 + n
        if n & 1:
            assert blob[at:at + 1] == b"\n"
            at += 1
        assert at % 2 == 0
        out.append((name.rstrip(b" "), int(mtime), int(uid), int(gid), int(mode, 8), data))
    assert at == len(blob)
    return out


MEMBERS = [(b"debian-binary", b"2.0\n"), (b"empty", b""), (b"odd", b"x" * 7), (b"even", b"y" * 8), (b"sixteen-bytes-ab", b"z"),
           (b"control.tar.gz", bytes(range(251))), (b"last-odd", b"123")]


def test_ar_round_trip(sb):
    assert len(MEMBERS[4][0]) == 16
    rc, blob = ar_write(sb, MEMBERS)
    assert rc == 0
    rc, mem = ar_parse(sb, blob)
    assert rc == 0
    assert [(n, s) for n, _, s in mem] == [(n, len(d)) for n, d in MEMBERS]
    for (n, off, size), (_, d) in zip(mem, MEMBERS):
        assert blob[off:off + size] == d and off % 2 == 0
    assert len(blob) % 2 == 0  # the padding byte after the last member is written too


def test_ar_layout_against_a_plain_parser(sb):
    rc, blob = ar_write(sb, MEMBERS, mtime=1445212800, mode=0o100644)
    assert rc == 0
    got = plain_ar(blob)
    assert got == [(n, 1445212800, 0, 0, 0o100644, d) for n, d in MEMBERS]
    h = blob[8:68]
    assert h == b"debian-binary   " + b"1445212800  " + b"0     " + b"0     " + b"100644  " + b"4         " + b"`\n"
    rc, blob = ar_write(sb, [], mtime=0)
    assert rc == 0 and blob == b"!<arch>\n"
    rc, blob = ar_write(sb, [(b"a", b"")], mtime=0, mode=0o644)
    assert rc == 0 and plain_ar(blob) == [(b"a", 0, 0, 0, 0o644, b"")]


def test_ar_refuses_what_the_reader_would_not_give_back(sb):
    assert ar_write(sb, [(b"seventeen-bytes-a", b"x")]) == (EINVAL, b"")
    assert ar_write(sb, [(b"ok", b"x"), (b"x" * 17, b"")])[0] == EINVAL
    assert ar_write(sb, [(b"", b"x")])[0] == EINVAL
    assert ar_write(sb, [(b"trailing ", b"x")])[0] == EINVAL
    assert ar_write(sb, [(b"a", b"x")], mtime=-1)[0] == EINVAL
    assert ar_write(sb, [(b"a", b"x")], mtime=10 ** 12)[0] == EINVAL
    assert ar_write(sb, [(b"a", b"x")], mtime=10 ** 12 - 1)[0] == 0


# ---- the walker -------------------------------------------------------------------------------------------------------

def walk(L, data, z, z_off, final):
    nch = len(z_off) - 1
    off = (ctypes.c_uint64 * (nch + 1))(*z_off)
    v = (ctypes.c_uint32 * (2 * nch))()
    L.sb_deflate_check(data, len(data), z, off, nch, 1 if final else 0, v)
    return [(v[2 * c], v[2 * c + 1]) for c in range(nch)]


def hold_safety(L, case):
    name, data, z, z_off, final, good = case[:6]
    verdicts = walk(L, data, z, z_off, final)
    nch = len(z_off) - 1
    for c, (status, at) in enumerate(verdicts):
        if status == S.TABLE:
            continue
        agrees = S.zlib_accepts(data, z, z_off, c, final and c == nch - 1)
        if status == S.OK:
            assert agrees, "%s: chunk %d accepted, zlib does not decode it to the chunk" % (name, c)
        if good:
            assert status == S.OK, "%s: chunk %d of an undamaged stream refused: status %d at %d" % (name, c, status, at)
            assert agrees, "%s: the case itself is not what zlib reads" % name
    return verdicts


def test_distance_bound(sb):
    assert sb.sb_distance_ok(32768, 65536) == 1 and sb.sb_distance_ok(32769, 65536) == 0
    assert sb.sb_distance_ok(32768, 32768) == 1 and sb.sb_distance_ok(32768, 32767) == 0
    assert sb.sb_distance_ok(1, 1) == 1 and sb.sb_distance_ok(1, 0) == 0


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_built_blocks(sb, case):
    verdicts = hold_safety(sb, case)
    print(case[0], verdicts)
    if case[6] is not None:
        assert verdicts == case[6]


@pytest.mark.parametrize("case", VALID, ids=[c[0] for c in VALID])
def test_zlib_streams_are_accepted(sb, case):
    name, data, z, z_off, final, good = case
    assert len(z_off) - 1 == S.nchunks_of(len(data))
    verdicts = hold_safety(sb, case)
    assert [s for s, _ in verdicts] == [S.OK] * len(verdicts)
    assert [at for _, at in verdicts] == [len(data[c * S.CHUNK:(c + 1) * S.CHUNK]) for c in range(len(verdicts))]


def test_the_valid_streams_hold_every_block_type():
    kinds = set()
    for name, data, z, z_off, final, good in VALID:
        for c in range(len(z_off) - 1):
            if z_off[c + 1] > z_off[c]:
                kinds.add((z[z_off[c]] >> 1) & 3)
    assert kinds == {0, 1, 2}  # stored (level 0), fixed (short inputs), dynamic


def test_damaged_streams_safety(sb):
    """Every damaged case; none is left out.  Prints what each one got."""
    assert len(DAMAGED) >= 1 + 64 + 32 + 40 - 8 + 3 + 4
    accepted = 0
    for case in DAMAGED:
        verdicts = hold_safety(sb, case)
        accepted += all(s == S.OK for s, _ in verdicts)
        print(case[0], verdicts)
    print("%d damaged cases, %d of them accepted in every chunk (zlib agreed on each)" % (len(DAMAGED), accepted))
    # the staged-byte cases change a byte the stream states: they cannot be accepted
    for case in DAMAGED:
        if case[0].startswith("staged_"):
            assert any(s != S.OK for s, _ in walk(sb, *case[1:5])), case[0]


def test_table_entries_outside_the_buffer(sb):
    name, data, z, z_off, final, good = VALID[-2]
    bad = list(z_off)
    bad[1] = bad[2] + 1  # descends: chunk 1's stretch would have a negative length
    v = walk(sb, data, z, bad, final)
    assert v[1][0] == S.TABLE
    bad = list(z_off)
    bad[-2] = bad[-1] + 5  # past the end of the buffer (whose size the table's last entry states)
    v = walk(sb, data, z, bad, final)
    assert v[-1][0] == S.TABLE and v[-2][0] == S.TABLE


def test_walker_under_asan_and_ubsan(tmp_path):
    """Host code only, in a program of its own (tests/asan_deflate_check.cpp): every case, each buffer on the heap at
    exactly its size."""
    exe = hostbuild.sanitized(["tests/asan_deflate_check.cpp"])
    cases = S.all_cases()
    blob = bytearray()
    for name, data, z, z_off, final, good in cases:
        blob += struct.pack("<QQQQ", len(data), len(z), len(z_off) - 1, 1 if final else 0) + data + z + struct.pack("<%dQ" % len(z_off), *z_off)
    inputs = tmp_path / "streams.bin"
    inputs.write_bytes(bytes(blob))
    out = hostbuild.run_sanitized(exe, [inputs])
    print(out.stdout[-400:])
    assert out.stdout.startswith("%d streams, " % len(cases))
