"""The .snap container on the CPU (snappy_amd/csrc/snap_core.h through tests/snap_host_harness.cpp): the ar parser on
every shape it refuses, ar's even-offset padding both ways, first-member and prefix matching, the suffix switch with the
reference's ".xz" message, and the order in which the audit reports mismatches.  Everything that needs a ctx -- open,
the decodes, audit and unpack on real packages -- is in tests/test_gpu_snap.py (snaphash_init needs a device)."""
import ctypes
import functools
import hashlib

import pytest

import snap_cases
import hostbuild

EINVAL, EFORMAT = -1, -9


@functools.lru_cache(maxsize=None)
def load_snap():
    """tests/snap_host_harness.cpp, loaded once a process with every prototype (it keeps no state between calls)."""
    L = hostbuild.shared("tests/snap_host_harness.cpp")
    L.sh_ar_parse.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t]
    L.sh_ar_pick.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int),
                             ctypes.c_char_p, ctypes.c_size_t]
    L.sh_audit.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
    return L


@pytest.fixture(scope="module")
def sh():
    return load_snap()


def parse(L, data):
    out = ctypes.create_string_buffer(1 << 16)
    rc = L.sh_ar_parse(data, len(data), out, len(out))
    if rc:
        return rc, out.value.decode()
    return 0, [(f[0], int(f[1]), int(f[2])) for f in (l.split("\t") for l in out.value.decode().splitlines())]


def pick(L, data, prefix):
    i, codec, why = ctypes.c_uint64(), ctypes.c_int(), ctypes.create_string_buffer(4096)
    rc = L.sh_ar_pick(data, len(data), prefix.encode(), ctypes.byref(i), ctypes.byref(codec), why, len(why))
    return rc, i.value, codec.value, why.value.decode()


def test_members_and_padding(sh):
    for n_ctl in (10, 11):  # the member in front of data.tar.gz even and odd: ar pads the odd one
        ctl, data = b"c" * n_ctl, b"d" * 5
        ar = snap_cases.ar_pack([("debian-binary", b"2.0\n"), ("control.tar.gz", ctl), ("data.tar.gz", data)])
        rc, mem = parse(sh, ar)
        assert rc == 0
        assert [m[0] for m in mem] == ["debian-binary", "control.tar.gz", "data.tar.gz"]
        for (name, off, size), want in zip(mem, (b"2.0\n", ctl, data)):
            assert ar[off:off + size] == want and off % 2 == 0
        # the last member's own padding byte may be missing
        assert parse(sh, ar[:-1] if len(data) & 1 else ar)[0] == 0
    assert parse(sh, b"!<arch>\n") == (0, [])
    # a name of all 16 bytes, and trailing spaces are all that is stripped
    rc, mem = parse(sh, snap_cases.ar_pack([("sixteen-byte-nam", b""), ("a b", b"x")]))
    assert rc == 0 and [m[0] for m in mem] == ["sixteen-byte-nam", "a b"]


def test_refused_shapes(sh):
    good = snap_cases.ar_pack([("control.tar.gz", b"cc"), ("data.tar.gz", b"dddd")])
    assert parse(sh, good)[0] == 0

    def bad(data):
        rc, why = parse(sh, data)
        assert rc == EFORMAT and why.startswith("ar: "), (rc, why)

    bad(b"")
    bad(b"!<arch>")                      # the magic cut off
    bad(b"!<arkh>\n" + good[8:])         # a wrong magic
    bad(good[:8 + 58] + b"`\r" + good[8 + 60:])   # a wrong fmag
    bad(good[:8 + 48] + b"2x        " + good[8 + 58:])  # a size that is not decimal
    bad(good[:8 + 48] + b"2 2       " + good[8 + 58:])  # digits after the spaces
    bad(good[:8 + 48] + b"          " + good[8 + 58:])  # no digit at all
    bad(good[:8 + 48] + b"0x2       " + good[8 + 58:])
    bad(good[:-1])                       # the last member runs past the end of the file
    bad(good[:8 + 60 + 2 + 30])          # the second header cut off by the end of the file
    bad(good + b"x")                     # one stray byte is a header cut off too


def test_first_member_with_the_prefix(sh):
    ar = snap_cases.ar_pack([("debian-binary", b"2.0\n"), ("data.tar.bz2", b"b"), ("control.tar.gz", b"c"), ("data.tar.gz", b"d"),
                             ("control.tar.bz2", b"e")])
    assert pick(sh, ar, "data.tar")[:3] == (0, 1, 1)      # the first of the two, and it is the bzip2 one
    assert pick(sh, ar, "control.tar")[:3] == (0, 2, 0)
    # a prefix match is all the reference asks: "data.tarball.gz" is taken for data.tar
    ar = snap_cases.ar_pack([("data.tarball.gz", b"d")])
    assert pick(sh, ar, "data.tar")[:3] == (0, 0, 0)
    # the prefix must be at the START of the name
    rc, _, _, why = pick(sh, snap_cases.ar_pack([("xdata.tar.gz", b"d")]), "data.tar")
    assert rc == EFORMAT and "data.tar" in why


def test_suffix_switch(sh):
    for name, want in (("data.tar.xz", EINVAL), ("data.tar", EINVAL), ("data.tar.lzma", EINVAL), ("data.tar.gz", 0), ("data.tar.bz2", 0)):
        rc, _, codec, why = pick(sh, snap_cases.ar_pack([(name, b"d")]), "data.tar")
        assert rc == want, name
        if want:
            assert why == "Can not handle " + name
        else:
            assert codec == (1 if name.endswith(".bz2") else 0)
    # the first match decides even when a later member could be read
    rc, i, _, why = pick(sh, snap_cases.ar_pack([("data.tar.xz", b"d"), ("data.tar.gz", b"d")]), "data.tar")
    assert (rc, i, why) == (EINVAL, 0, "Can not handle data.tar.xz")
    rc, _, _, why = pick(sh, snap_cases.ar_pack([("debian-binary", b"2.0\n")]), "control.tar")
    assert rc == EFORMAT and "control.tar" in why


# ---- the audit's comparison ----------------------------------------------------------------------------------------------

DIG = {n: hashlib.sha512(n.encode()).hexdigest() for n in ("a", "b", "old")}


def audit(L, recs, mem):
    r = "".join("%s\t%o\t%d\t%s\n" % x for x in recs).encode()
    m = "".join("%s\t%s\t%o\t%d\t%s\n" % x for x in mem).encode()
    name = ctypes.create_string_buffer(4096)
    return L.sh_audit(r, m, name, len(name)), name.value.decode()


RECS = [("d", 0o040755, -1, "-"), ("d/a", 0o100644, 1, DIG["a"]), ("d/b", 0o100755, 2, DIG["b"]), ("l", 0o120777, -1, "-")]
MEM = [(".", "5", 0o755, 0, "-"), ("d", "5", 0o755, 0, "-"), ("d/a", "0", 0o644, 1, DIG["a"]), ("d/b", "0", 0o755, 2, DIG["b"]),
       ("l", "2", 0o777, 0, "-")]


def test_audit_agrees(sh):
    assert audit(sh, RECS, MEM) == (0, "")
    assert audit(sh, [], [(".", "5", 0o755, 0, "-")]) == (0, "")
    # the LAST member of a name is what counts: an earlier one may be anything
    early = [("d/a", "0", 0o600, 3, DIG["old"])]
    assert audit(sh, RECS, MEM[:1] + early + MEM[1:]) == (0, "")
    assert audit(sh, RECS, MEM + early) == (5, "d/a")


def test_audit_kinds(sh):
    def mem_with(i, **kw):
        m = list(MEM)
        t = dict(zip(("name", "type", "mode", "size", "dig"), m[i]), **kw)
        m[i] = (t["name"], t["type"], t["mode"], t["size"], t["dig"])
        return m

    assert audit(sh, RECS, MEM[:2] + MEM[3:]) == (1, "d/a")                  # no member of the record's name
    assert audit(sh, RECS[:1] + RECS[2:], MEM) == (2, "d/a")                 # a member no record has
    assert audit(sh, RECS, mem_with(2, size=2)) == (3, "d/a")
    assert audit(sh, RECS, mem_with(2, dig=DIG["b"])) == (4, "d/a")
    assert audit(sh, RECS, mem_with(2, mode=0o600)) == (5, "d/a")
    assert audit(sh, RECS, mem_with(2, type="2")) == (5, "d/a")             # the type letter is part of the mode
    assert audit(sh, RECS, mem_with(1, mode=0o700)) == (5, "d")
    assert audit(sh, RECS, mem_with(2, mode=0o4644)) == (0, "")             # the low nine bits only
    # a record of a regular file without a size
    assert audit(sh, [("d/a", 0o100644, -1, DIG["a"])], [MEM[2]]) == (3, "d/a")


def test_audit_order(sh):
    """The records in yaml order first -- within one record mode, then size, then digest -- and only then the members no
    record has, in tar order."""
    m = list(MEM)
    m[3] = ("d/b", "0", 0o700, 9, DIG["a"])      # mode, size and digest all wrong: the mode is reported
    assert audit(sh, RECS, m) == (5, "d/b")
    m[3] = ("d/b", "0", 0o755, 9, DIG["a"])
    assert audit(sh, RECS, m) == (3, "d/b")
    m[3] = ("d/b", "0", 0o755, 2, DIG["a"])
    assert audit(sh, RECS, m) == (4, "d/b")
    # an unrecorded member EARLY in the tar and a bad record LATE in the yaml: the record is reported
    extra = [("aaa", "0", 0o644, 0, DIG["a"])]
    assert audit(sh, RECS, MEM[:1] + extra + MEM[1:4] + [("l", "0", 0o777, 0, "-")]) == (5, "l")
    # a missing member late in the yaml against an unrecorded member early in the tar
    assert audit(sh, RECS, MEM[:1] + extra + MEM[1:4]) == (1, "l")
    # two unrecorded members: the first in tar order
    assert audit(sh, RECS, MEM + [("zz", "5", 0o755, 0, "-")] + extra) == (2, "zz")
    # two failing records: the first in yaml order, whatever the tar order
    m = [MEM[0], MEM[1], ("d/b", "0", 0o755, 3, DIG["b"]), ("d/a", "0", 0o644, 2, DIG["a"]), MEM[4]]
    assert audit(sh, RECS, m) == (3, "d/a")
