"""The tar reader on the CPU (snappy_amd/csrc/tar_core.h through tests/tar_host_harness.cpp): every stream of
tests/tar_cases.py -- the good ones member by member against Python's tarfile, the bad ones code by code -- and for EVERY
result, good, bad or mutated, the invariant the member writer and the SHA-512 job tables rely on: an entry's data_off is
within the stream and its size within what is left behind it.  The harness checks that in C++ on each call and answers 77
where it fails, whatever tar_read returned.

A negative base-256 mode (all ones was once read as 07777) is REFUSED with EFORMAT, not masked: tar_octal refuses a
negative base-256 value in any field.

The same streams through the device entry points are in tests/test_gpu_tar_edges.py."""
import ctypes
import functools
import struct

import pytest

import tar_cases as T
import hostbuild

INVARIANT_BROKEN = 77
SWEEP_CAP = 1500000  # runs of tar_read in the mutation sweep (a run is about a microsecond)

GOOD = T.good_cases()
BAD = T.bad_cases()


@functools.lru_cache(maxsize=None)
def load_th():
    """tests/tar_host_harness.cpp, loaded once a process with every prototype (it keeps no state between calls)."""
    L = hostbuild.shared("tests/tar_host_harness.cpp")
    L.th_tar_read.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t]
    L.th_sweep.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t, ctypes.c_uint64,
                           ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    L.th_go_clean.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    return L


@pytest.fixture(scope="module")
def th():
    return load_th()


def tar_read(L, tar):
    """-> (code, members as tar_cases expects them, last_regular_members, why)"""
    out = ctypes.create_string_buffer(1 << 16)
    rc = L.th_tar_read(tar, len(tar), out, len(out))
    unhex = lambda h: b"" if h == "-" else bytes.fromhex(h)
    ents, reg, why = [], None, ""
    for line in out.value.decode().split("\n"):
        f = line.split("\t")
        if f[0] == "reg":
            reg = [int(k) for k in f[1:]]
        elif f[0] == "why":
            why = f[1]
        elif len(f) == 6:
            ents.append((unhex(f[0]), f[1], int(f[2], 8), int(f[3]), int(f[4]), unhex(f[5])))
    return rc, ents, reg, why


def test_case_names_are_unique():
    names = [c[0] for c in GOOD + BAD]
    assert len(set(names)) == len(names)
    assert all(len(c[1]) < 8192 for c in GOOD + BAD)
    assert all(code in (T.EFORMAT, T.ECONTENT) for _, _, code in BAD)


@pytest.mark.parametrize("case", GOOD, ids=[c[0] for c in GOOD])
def test_good_case_members(th, case):
    name, tar, want = case
    rc, ents, reg, why = tar_read(th, tar)
    assert rc == 0, (rc, why)
    assert len(ents) == len(want), (ents, want)
    for k, (g, w) in enumerate(zip(ents, want)):
        for field, a, b in zip(("name", "type", "mode", "size", "data_off", "linkname"), g, w):
            assert a == b, (k, field, a, b)
        if g[1] == "0":
            assert g[4] + g[3] <= len(tar)
    assert reg == T.last_regular(want)


def test_what_the_good_cases_pin():
    """Spot checks that the expectations themselves (mostly tarfile's) say what the case is for."""
    want = {n: w for n, _, w in GOOD}
    assert [m[0] for m in want["ustar_name_99_100_101"]] == [b"a" * 99, b"b" * 100, b"pp/" + b"c" * 98]
    assert len(want["ustar_prefix_155"][0][0]) == 256
    assert want["pax_size_overrides_header"][0][3] == 513 and want["pax_size_overrides_header"][1][4] == 512 + 512 + 512 + 1024 + 512
    assert want["x_then_L"][0][0] == b"from-pax" and want["L_then_x"][0][0] == b"from-gnu"
    assert want["K_then_x_linkpath"][0][5] == b"link-gnu"
    assert want["pax_size_across_L"][0][0] == b"a-long-name" and want["pax_size_across_L"][0][3] == 5
    assert want["pax_size_across_x"][0][0] == b"second" and want["pax_size_across_x"][0][3] == 5
    assert [m[0] for m in want["override_does_not_leak"]] == [b"renamed", b"renamed-too", b"m3", b"l4"]
    assert [m[3] for m in want["override_does_not_leak"]] == [1, 2, 3, 0] and want["override_does_not_leak"][3][5] == b"own"
    assert [m[1] for m in want["type_nul_and_7"]] == ["0", "0"]
    assert [(m[1], m[3]) for m in want["dir_and_symlink_with_size"]] == [("5", 0), ("2", 0), ("0", 1)]
    assert want["base256_size"][0][3] == 5 and want["base256_mode"][0][2] == 0o755
    assert [m[0] for m in want["clean_names"]] == [b"a/b/c", b"a", b"/abs/x", b"y"]
    assert T.last_regular(want["duplicate_last_wins"]) == [1, 2]
    assert T.last_regular(want["regular_then_symlink_then_dir"]) == []
    for n in ("end_at_eof", "end_one_zero_block", "end_one_zero_block_and_a_bit", "end_two_zero_blocks", "end_two_zero_blocks_then_junk"):
        assert [m[0] for m in want[n]] == [b"one"]


@pytest.mark.parametrize("case", BAD, ids=[c[0] for c in BAD])
def test_bad_case_code(th, case):
    name, tar, code = case
    rc, ents, reg, why = tar_read(th, tar)
    print("%s: rc %d (%s), %d entries before it: %s" % (name, rc, why, len(ents), [(e[0], e[3], e[4]) for e in ents]))
    assert rc != INVARIANT_BROKEN, "an entry's extent leaves the stream of %d bytes: %s" % (len(tar), [(e[0], e[3], e[4]) for e in ents])
    assert rc == code, (rc, why)
    assert why.startswith("tar: ")


def test_mutation_sweep_keeps_every_extent_inside(th):
    """Each bit of each header block and of each PAX/GNU body of each good case flipped, one at a time, and each numeric
    header field set to 0, all '7', all 0xff and 0x80 + zeros -- headers with the checksum as it was and put right again.
    One thing is asked of each result: the call returns and every entry's extent is inside the stream."""
    plans = [(name, tar, T.regions(tar)) for name, tar, _ in GOOD]
    assert sum(1 for _, _, r in plans for x in r if not x[2]) >= 15  # the PAX and GNU bodies were found
    planned = sum(2 * 8 * ln + (44 if hd else 0) for _, _, r in plans for _, ln, hd in r)
    stride = 1
    while planned // stride > SWEEP_CAP:
        stride += 2  # (odd: every bit position of a byte is still reached)
    total = 0
    for name, tar, reg in plans:
        if not reg:
            continue
        flat = (ctypes.c_uint64 * (3 * len(reg)))(*[v for r in reg for v in r])
        runs, where = ctypes.c_uint64(), ctypes.c_uint64()
        rc = th.th_sweep(tar, len(tar), flat, len(reg), stride, ctypes.byref(runs), ctypes.byref(where))
        total += runs.value
        assert rc == 0, "%s: a mutation at byte %d gives an entry outside the stream" % (name, where.value)
    print("mutation sweep: %d runs of tar_read over %d archives, every bit in %d" % (total, len(plans), stride))
    assert total >= min(planned // stride, SWEEP_CAP) // 2


def test_go_clean_against_normpath(th):
    table = T.clean_table()
    assert len(table) >= 300
    out = ctypes.create_string_buffer(4096)
    for p, want in table:
        th.th_go_clean(p, len(p), out, len(out))
        assert out.value == want, (p, out.value, want)
    # and the cases' own restatement agrees with the table
    for p, want in table:
        assert T.clean(p) == want, p


def test_tar_read_under_asan_and_ubsan(tmp_path):
    """Host code only, in a program of its own (tests/asan_tarread.cpp): every case, and the sweep's field values on every
    block of every case, each stream in a heap buffer of exactly its size."""
    exe = hostbuild.sanitized(["tests/asan_tarread.cpp"])
    inputs = tmp_path / "archives.bin"
    archives = [c[1] for c in BAD + GOOD]
    inputs.write_bytes(b"".join(struct.pack("<Q", len(a)) + a for a in archives))
    out = hostbuild.run_sanitized(exe, [inputs])
    print(out.stdout[-400:])
    assert out.stdout.startswith("%d archives, " % len(archives)) and out.stdout.rstrip().endswith(" 0 broke the invariant")
