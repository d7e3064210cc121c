"""The .snap container's .xz route on the CPU (snappy_amd/csrc/snap_core.h through tests/snap_xz_host_harness.cpp): the
member lookup with ".xz" allowed over the name table of tests/test_snap_host.py, first-member-wins with the .xz member in
front of a .gz one and behind it, ar_pick itself still refusing ".xz", and the container's writer with the data member's
three names.  What needs a ctx -- sessions and builds on real packages -- is in tests/test_gpu_snap_xz.py and
tests/test_gpu_snap_build_codecs.py."""
import ctypes
import functools

import pytest

import hostbuild
import snap_cases

EINVAL, EFORMAT = -1, -9
GZ, BZ2, XZ = 0, 1, 2
WRAPPER = -1  # sx_ar_pick: ar_pick itself


@functools.lru_cache(maxsize=None)
def load_snap_xz():
    """tests/snap_xz_host_harness.cpp, loaded once a process with every prototype (it keeps no state between calls)."""
    L = hostbuild.shared("tests/snap_xz_host_harness.cpp")
    L.sx_ar_pick.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64),
                             ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_size_t]
    L.sx_ar_write.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    L.sx_ar_header.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_char_p]
    L.sx_ar_parse.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t]
    return L


@pytest.fixture(scope="module")
def sx():
    return load_snap_xz()


def pick(L, members, prefix, xz_allowed):
    data = snap_cases.ar_pack(members)
    i, codec, why = ctypes.c_uint64(), ctypes.c_int(-7), ctypes.create_string_buffer(4096)
    rc = L.sx_ar_pick(data, len(data), prefix.encode(), xz_allowed, ctypes.byref(i), ctypes.byref(codec), why, len(why))
    return rc, i.value, codec.value, why.value.decode()


# test_snap_host.py's name table, with what the lookup answers when ".xz" is allowed
NAMES = [("data.tar.gz", 0, GZ), ("data.tar.bz2", 0, BZ2), ("data.tar.xz", 0, XZ), ("data.tar.lzma", EINVAL, None), ("data.tar", EINVAL, None)]


def test_suffix_switch_with_xz_allowed(sx):
    for name, want, codec in NAMES:
        rc, i, got, why = pick(sx, [(name, b"d")], "data.tar", 1)
        assert (rc, i) == (want, 0), name
        if want:
            assert why == "Can not handle " + name
        else:
            assert got == codec, name
    # the control member takes the same switch
    assert pick(sx, [("debian-binary", b"2.0\n"), ("control.tar.xz", b"c")], "control.tar", 1)[:3] == (0, 1, XZ)
    # no member of the prefix: the format error, allowed or not
    for allowed in (1, 0, WRAPPER):
        rc, _, _, why = pick(sx, [("debian-binary", b"2.0\n")], "control.tar", allowed)
        assert rc == EFORMAT and "control.tar" in why
    # the suffix is a suffix: ".xz" in the middle of a name is nothing
    rc, _, _, why = pick(sx, [("data.tar.xz.old", b"d")], "data.tar", 1)
    assert (rc, why) == (EINVAL, "Can not handle data.tar.xz.old")


def test_first_member_wins_with_xz_in_front_and_behind(sx):
    front = [("debian-binary", b"2.0\n"), ("data.tar.xz", b"x"), ("control.tar.gz", b"c"), ("data.tar.gz", b"d")]
    behind = [("debian-binary", b"2.0\n"), ("data.tar.gz", b"d"), ("control.tar.gz", b"c"), ("data.tar.xz", b"x")]
    assert pick(sx, front, "data.tar", 1)[:3] == (0, 1, XZ)       # the .xz one, not the readable .gz one behind it
    assert pick(sx, behind, "data.tar", 1)[:3] == (0, 1, GZ)      # and the .gz one when it comes first
    assert pick(sx, front, "control.tar", 1)[:3] == (0, 2, GZ)
    # not allowed: the first match still decides, and it is the refusal
    for allowed in (0, WRAPPER):
        rc, i, _, why = pick(sx, front, "data.tar", allowed)
        assert (rc, i, why) == (EINVAL, 1, "Can not handle data.tar.xz")
        assert pick(sx, behind, "data.tar", allowed)[:3] == (0, 1, GZ)
    # .bz2 and .xz beside each other
    assert pick(sx, [("data.tar.bz2", b"b"), ("data.tar.xz", b"x")], "data.tar", 1)[:3] == (0, 0, BZ2)
    assert pick(sx, [("data.tar.xz", b"x"), ("data.tar.bz2", b"b")], "data.tar", 1)[:3] == (0, 0, XZ)


def test_ar_pick_itself_still_refuses_xz(sx):
    for name, want, codec in NAMES:
        rc, i, got, why = pick(sx, [(name, b"d")], "data.tar", WRAPPER)
        if name.endswith(".xz"):
            assert (rc, why) == (EINVAL, "Can not handle data.tar.xz")
        else:
            assert rc == want and (want or got == codec), name
        assert pick(sx, [(name, b"d")], "data.tar", 0)[0::3] == (rc, why)   # the variant with "not allowed" is the wrapper
    assert pick(sx, [("control.tar.xz", b"c")], "control.tar", WRAPPER)[0::3] == (EINVAL, "Can not handle control.tar.xz")


def parse(L, data):
    out = ctypes.create_string_buffer(1 << 16)
    rc = L.sx_ar_parse(data, len(data), out, len(out))
    assert rc == 0, out.value
    return [(f[0], int(f[1]), int(f[2])) for f in (l.split("\t") for l in out.value.decode().splitlines())]


MTIME = 1445212800


@pytest.mark.parametrize("data_name", ["data.tar.gz", "data.tar.bz2", "data.tar.xz"])
def test_writer_with_the_data_members_names(sx, data_name):
    assert len(data_name) <= 16
    h = ctypes.create_string_buffer(60)
    assert sx.sx_ar_header(data_name.encode(), MTIME, 0o100644, 12345, h) == 0
    assert h.raw == b"%-16s%-12d%-6d%-6d%-8s%-10d`\n" % (data_name.encode(), MTIME, 0, 0, b"100644", 12345)
    # a container as snaphash_snap_build lays it out, the control member of odd and of even length
    for n_ctl in (10, 11):
        members = [("debian-binary", 4), ("_click-binary", 4), ("control.tar.gz", n_ctl), (data_name, 7)]
        spec = "".join("%s\t%d\n" % m for m in members).encode()
        out, n = ctypes.create_string_buffer(4096), ctypes.c_size_t()
        assert sx.sx_ar_write(spec, MTIME, 0o100644, out, len(out), ctypes.byref(n)) == 0
        ar = out.raw[:n.value]
        assert len(ar) % 2 == 0
        # the builder of the test packages writes the same bytes (its mtime field is 0: compare with it patched in)
        want = snap_cases.ar_pack([(nm, bytes([ord("a") + k]) * size) for k, (nm, size) in enumerate(members)])
        got = parse(sx, ar)
        assert [(m[0], m[2]) for m in got] == members
        norm = bytearray(ar)
        for k, (name, off, size) in enumerate(got):
            assert off % 2 == 0 and ar[off:off + size] == bytes([ord("a") + k]) * size
            assert ar[off - 60:off - 44] == b"%-16s" % name.encode()
            assert ar[off - 44:off - 32] == b"%-12d" % MTIME
            norm[off - 44:off - 32] = b"%-12d" % 0
        assert bytes(norm) == want
        # and the lookups find the members that went in
        assert pick_bytes(sx, ar, "data.tar", 1)[:2] == (0, 3)
        assert pick_bytes(sx, ar, "control.tar", 1)[:3] == (0, 2, GZ)


def pick_bytes(L, data, prefix, xz_allowed):
    i, codec, why = ctypes.c_uint64(), ctypes.c_int(-7), ctypes.create_string_buffer(4096)
    rc = L.sx_ar_pick(data, len(data), prefix.encode(), xz_allowed, ctypes.byref(i), ctypes.byref(codec), why, len(why))
    return rc, i.value, codec.value, why.value.decode()


def test_names_the_header_cannot_hold(sx):
    h = ctypes.create_string_buffer(60)
    assert sx.sx_ar_header(b"data.tar.bz2", 0, 0o100644, 0, h) == 0
    assert sx.sx_ar_header(b"sixteen-byte-nam", 0, 0o100644, 0, h) == 0
    assert sx.sx_ar_header(b"seventeen-byte-nm", 0, 0o100644, 0, h) == EINVAL
    assert sx.sx_ar_header(b"", 0, 0o100644, 0, h) == EINVAL
