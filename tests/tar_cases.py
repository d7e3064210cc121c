"""Hand-made tar streams for the tar reader (snappy_amd/csrc/tar_core.h): tests/test_tar_host.py runs them on the CPU,
tests/test_gpu_tar_edges.py sends some through the device entry points.  Plain Python, deterministic, no file read.  Every
header is put together byte by byte here; what a GOOD stream holds is then read back with Python's tarfile, the independent
reference, except where tarfile and Go's archive/tar are known to differ -- those expectations are written by hand and
say so.  A number of 2^64's scale is only ever a decimal string or 12 bytes of a header: no case is larger than a few KiB.

An expected member is (name after filepath.Clean, type '0'/'2'/'5', mode & 07777, size, data offset, link name), names as
bytes.

Rooted names: the project keeps "/abs/x" rooted in the member list (Clean keeps a leading "/"), and the member writer joins
it under the target -- the reference's filepath.Join(targetDir, name) keeps it inside the same way.

A builder, not a test."""
import io
import posixpath
import tarfile

EFORMAT, ECONTENT = -9, -10
USTAR = b"ustar\x0000"
GNU = b"ustar  \x00"


def clean(name):
    """filepath.Clean for the names used here, from posixpath.normpath: Go collapses a leading "//" that POSIX keeps."""
    r = posixpath.normpath(name) if name else b"."
    return b"/" + r.lstrip(b"/") if r.startswith(b"//") else r


def set_checksum(h, signed=False, delta=0):
    h[148:156] = b" " * 8
    s = sum(b - 256 if signed and b >= 128 else b for b in h) + delta
    h[148:156] = b"%06o\x00 " % s
    return h


def header(name, typ=b"0", size=0, mode=0o644, link=b"", magic=USTAR, prefix=b"", size_field=None, mode_field=None, signed=False,
           delta=0):
    """One 512-byte header block.  size_field / mode_field: the raw bytes of the field in place of the octal number."""
    assert len(name) <= 100 and len(link) <= 100 and len(prefix) <= 155
    h = bytearray(512)
    h[0:len(name)] = name
    h[100:108] = mode_field if mode_field is not None else b"%07o\x00" % mode
    h[108:116] = h[116:124] = b"0000000\x00"
    h[124:136] = size_field if size_field is not None else b"%011o\x00" % size
    h[136:148] = b"%011o\x00" % 0
    h[156:157] = typ
    h[157:157 + len(link)] = link
    h[257:257 + len(magic)] = magic
    h[345:345 + len(prefix)] = prefix
    return bytes(set_checksum(h, signed, delta))


def pad(data):
    return data + bytes(-len(data) % 512)


def member(name, data=b"", **kw):
    """A regular member (or whatever typ says) with its data padded; the header's size is len(data) unless given."""
    kw.setdefault("size", len(data))
    return header(name, **kw) + pad(data)


def record(key, value):
    """One PAX record "<len> key=value\\n", the length counting itself."""
    body = b" " + key + b"=" + value + b"\n"
    n = len(body) + 1
    while len(b"%d" % n) + len(body) != n:
        n = len(b"%d" % n) + len(body)
    return b"%d" % n + body


def pax(*records, **kw):
    """An 'x' header with these records (bytes taken as they are) as its body."""
    return member(b"PaxHeaders/x", b"".join(records), typ=b"x", **kw)


def gnu_long(typ, value):
    return member(b"././@LongLink", value + b"\x00", typ=typ, magic=GNU)


END = bytes(1024)
B256_5 = b"\x80" + bytes(10) + b"\x05"


def via_tarfile(tar):
    out = []
    with tarfile.open(fileobj=io.BytesIO(tar), mode="r:") as t:
        for m in t:
            typ = "0" if m.isreg() else "5" if m.isdir() else "2" if m.issym() else m.type.decode("latin-1")
            enc = lambda s: s.encode("utf-8", "surrogateescape")
            out.append((clean(enc(m.name)), typ, m.mode & 0o7777, m.size if m.isreg() else 0, m.offset_data, enc(m.linkname)))
    return out


def good_cases():
    """-> [(name, tar bytes, expected members)]"""
    cases = []

    def add(name, tar, expect=None):
        cases.append((name, tar, via_tarfile(tar) if expect is None else expect))

    # ustar names at the limits of the 100-byte name and the 155-byte prefix
    n99, n100 = b"a" * 99, b"b" * 100
    add("ustar_name_99_100_101", member(n99, b"x") + member(n100, b"yy") + member(b"c" * 98, b"zzz", prefix=b"pp") + END)
    add("ustar_prefix_155", member(b"n" * 100, b"deep", prefix=b"d" * 155) + END)
    # GNU 'L' and 'K'
    long_name, long_link = b"long/" + b"n" * 150, b"target/" + b"t" * 150
    add("gnu_L", gnu_long(b"L", long_name) + member(b"short", b"data", magic=GNU) + END)
    add("gnu_K_L_symlink", gnu_long(b"K", long_link) + gnu_long(b"L", long_name) + header(b"short", b"2", link=b"t", mode=0o777, magic=GNU) + END)
    # PAX path, linkpath, size
    add("pax_path", pax(record(b"path", b"pax/" + b"p" * 120)) + member(b"short", b"data") + END)
    add("pax_linkpath", pax(record(b"linkpath", long_link), record(b"path", b"pl")) + header(b"short", b"2", link=b"t", mode=0o777) + END)
    add("pax_size_overrides_header", pax(record(b"size", b"513")) + member(b"sz", b"s" * 513, size=7) + member(b"after", b"a") + END)
    add("pax_unknown_keys_and_binary_value", pax(record(b"mtime", b"1.5"), record(b"SCHILY.xattr.user.k", b"v\x00w"), record(b"path", b"u")) +
        member(b"short", b"q") + END)
    # PAX and GNU in front of one member: the one that comes first names it (tarfile, and the archive/tar of the
    # reference's time, read the next header recursively and apply the outer one last; today's archive/tar lets the GNU
    # name win in both orders, so "x_then_L" is where the two Go readers differ -- tarfile's answer is pinned)
    add("x_then_L", pax(record(b"path", b"from-pax")) + gnu_long(b"L", b"from-gnu") + member(b"short", b"1") + END)
    add("L_then_x", gnu_long(b"L", b"from-gnu") + pax(record(b"path", b"from-pax")) + member(b"short", b"1") + END)
    add("K_then_x_linkpath", gnu_long(b"K", b"link-gnu") + pax(record(b"linkpath", b"link-pax")) + header(b"s", b"2", link=b"t") + END)
    # a PAX size belongs to the member, not to the 'L' or the 'x' between
    add("pax_size_across_L", pax(record(b"size", b"5")) + gnu_long(b"L", b"a-long-name") + member(b"short", b"12345", size=0) + END)
    add("pax_size_across_x", pax(record(b"size", b"5")) + pax(record(b"path", b"second")) + member(b"short", b"12345", size=0) + END)
    # an override does not leak onto the member after next
    add("override_does_not_leak", pax(record(b"path", b"renamed"), record(b"linkpath", b"ln"), record(b"size", b"1")) + member(b"m1", b"1") +
        gnu_long(b"L", b"renamed-too") + member(b"m2", b"22") + member(b"m3", b"333") + header(b"l4", b"2", link=b"own") + END)
    # type NUL and type '7' are regular files
    add("type_nul_and_7", member(b"old", b"o", typ=b"\x00") + member(b"cont", b"c", typ=b"7") + END)
    # a directory and a symlink whose size field is not 0: neither has data
    add("dir_and_symlink_with_size", header(b"d/", b"5", size=512, mode=0o755) + header(b"l", b"2", size=1000, link=b"d") + member(b"d/f", b"f") + END)
    for n in (0, 1, 511, 512, 513):
        add("size_%d" % n, member(b"f", (bytes(range(251)) * 3)[:n]) + member(b"g", b"g") + END)
    add("base256_size", member(b"b256", b"12345", size_field=B256_5, magic=GNU) + END)
    add("base256_mode", member(b"b256m", b"1", mode_field=b"\x80" + bytes(5) + b"\x01\xed", magic=GNU) + END)
    # old V7: no magic, and the prefix field is not a prefix.  BY HAND: tarfile joins the prefix field whatever the magic
    # says; archive/tar reads it only behind "ustar\0".
    add("v7_junk_prefix", member(b"v7file", b"seven", magic=b"", prefix=b"junk-not-a-prefix") + END,
        [(b"v7file", "0", 0o644, 5, 512, b"")])
    # a header whose checksum field holds the sum of SIGNED bytes
    add("signed_checksum", member(b"caf\xc3\xa9-\xff\xfe", b"s", signed=True) + END)
    # the end of the archive in each form
    one = member(b"one", b"1")
    add("end_at_eof", one)
    add("end_one_zero_block", one + bytes(512))
    add("end_one_zero_block_and_a_bit", one + bytes(512) + b"\x01" * 100)
    add("end_two_zero_blocks", one + END)
    add("end_two_zero_blocks_then_junk", one + END + b"junk" * 300)  # nothing behind the second zero block is looked at
    add("empty_stream", b"", [])  # BY HAND: tarfile calls an empty file an error, archive/tar an empty archive
    add("only_zero_blocks", END, [])
    # duplicates and replacements
    add("duplicate_last_wins", member(b"dup", b"first") + member(b"other", b"o") + member(b"./dup", b"second!") + END)
    add("regular_then_symlink_then_dir", member(b"rs", b"r") + member(b"rd", b"r") + header(b"rs", b"2", link=b"x") + header(b"rd/", b"5", mode=0o755) + END)
    # names Clean changes; the rooted one stays rooted (module docstring)
    add("clean_names", member(b"./a//b/./c", b"c") + header(b"a/", b"5", mode=0o755) + member(b"/abs/x", b"x") + member(b"x/../y", b"y") + END)
    return cases


def last_regular(expected):
    """last_regular_members restated: the indices of the last member of every name, where that one is a regular file."""
    last = {}
    for k, m in enumerate(expected):
        last[m[0]] = k
    return sorted(k for k in last.values() if expected[k][1] == "0")


def regions(tar):
    """The header blocks and the PAX/GNU bodies of a GOOD stream, as (offset, length, is_header), by the layout rules alone."""
    out, at, pax_size = [], 0, None
    while at + 512 <= len(tar) and any(tar[at:at + 512]):
        f = tar[at + 124:at + 136]
        size = int.from_bytes(f[1:], "big") if f[0] & 0x80 else int(f.rstrip(b" \x00") or b"0", 8)
        typ = tar[at + 156:at + 157]
        out.append((at, 512, 1))
        if typ in b"xLK":
            out.append((at + 512, size, 0))
            if typ == b"x":
                for rec in tar[at + 512:at + 512 + size].split(b"\n"):
                    if b" size=" in rec:
                        pax_size = int(rec.split(b"=")[1])
        else:
            if pax_size is not None:
                size, pax_size = pax_size, None
            if typ not in b"0\x007":
                size = 0
        at += 512 + (size + 511) // 512 * 512
    return out


def unpackable(name):
    """Good cases that describe a tree an unpack can create under a target, for the GPU tests: no rooted name, no stream
    that is no archive to tarfile or that tarfile names differently, and not the symlink over an existing file (os.Symlink
    fails with EEXIST in UnpackTar, and symlink() here, where tarfile unlinks first)."""
    return name not in ("clean_names", "empty_stream", "only_zero_blocks", "v7_junk_prefix", "regular_then_symlink_then_dir")


def bad_cases():
    """-> [(name, tar bytes, code)]"""
    cases = []

    def add(name, tar, code=EFORMAT):
        cases.append((name, tar, code))

    def raw_pax(body):
        return pax(body)

    # PAX "size": anything that is not a non-negative decimal int64 in full.  The record stands in front of an EMPTY member
    # followed by the end-of-archive blocks: with (size + 511) & ~511 wrapping to 0 this was accepted, the member's size
    # 2^64-1 with its data offset inside the stream.
    for label, v in (("2^64-1", b"18446744073709551615"), ("-1", b"-1"), ("huge", b"99999999999999999999999"), ("2^64-511", b"%d" % (2**64 - 511)),
                     ("2^63", b"%d" % 2**63), ("12abc", b"12abc"), ("empty", b""), ("plus", b"+1"), ("blank", b" 1")):
        add("pax_size_" + label, pax(record(b"size", v)) + member(b"victim") + END)
    add("pax_size_2^63-1", pax(record(b"size", b"%d" % (2**63 - 1))) + member(b"victim") + END)  # a legal number: "truncated member"
    # PAX record lengths
    ok13 = b"13 path=abcd\n"
    assert record(b"path", b"abcd") == ok13
    add("pax_len_wraps_behind_a_valid_record", raw_pax(ok13 + b"18446744073709551603 path=q\n") + member(b"m") + END)
    add("pax_len_0", raw_pax(b"0 path=a\n") + member(b"m") + END)
    add("pax_len_below_own_minimum", raw_pax(b"3 a=\n") + member(b"m") + END)
    add("pax_len_short_by_one", raw_pax(b"12 path=abcd\n") + member(b"m") + END)
    add("pax_len_one_beyond_body", raw_pax(b"14 path=abcd\n") + member(b"m") + END)
    add("pax_len_near_2^64", raw_pax(b"18446744073709551615 path=q\n") + member(b"m") + END)
    add("pax_len_not_digits", raw_pax(b"1e1 path=abcd\n") + member(b"m") + END)
    add("pax_no_newline", raw_pax(b"13 path=abcdX") + member(b"m") + END)
    add("pax_no_equals", raw_pax(b"9 pathab\n") + member(b"m") + END)
    add("pax_no_space", raw_pax(b"13path=abcde\n") + member(b"m") + END)
    add("pax_empty_key", raw_pax(b"6 =ab\n") + member(b"m") + END)
    add("pax_trailing_nuls", raw_pax(ok13 + bytes(3)) + member(b"m") + END)
    # NUL in a PAX path: "./z\0/.." came out as the name "." with the NUL inside; archive/tar refuses NUL in these values
    add("pax_path_with_nul", pax(record(b"path", b"./z\x00/..")) + member(b"m") + END)
    add("pax_linkpath_with_nul", pax(record(b"linkpath", b"a\x00b")) + header(b"l", b"2", link=b"t") + END)
    # the stream ends where it must not
    add("header_cut_at_511", member(b"ok", b"1") + header(b"cut")[:511])
    add("padded_data_one_byte_short", (member(b"m", b"d" * 513))[:-1])
    # the data ends exactly at the end of the stream, its padding missing: refused, AS TARFILE DOES ("unexpected end of
    # data").  archive/tar's Next returns io.EOF where the padding is absent altogether, i.e. would end quietly; the
    # project keeps the stricter reading it always had.
    add("data_ends_at_eof_without_padding", header(b"m", size=5) + b"12345")
    add("data_cut", header(b"m", size=600) + b"x" * 512)
    add("checksum_off_by_one", member(b"m", b"1", delta=1) + END)
    add("checksum_off_by_minus_one", member(b"m", b"1", delta=-1) + END)
    add("size_non_octal_digit", member(b"m", size_field=b"00000000008\x00") + END)
    add("size_digits_after_blank", member(b"m", size_field=b"0000 000001\x00") + END)
    add("size_eleven_7s", member(b"m", size_field=b"77777777777\x00") + END)
    add("size_twelve_7s", member(b"m", size_field=b"777777777777") + END)
    add("b256_size_negative", member(b"m", size_field=b"\xff" * 12, magic=GNU) + END)
    add("b256_size_2^63", member(b"m", size_field=b"\x80\x00\x00\x00\x80" + bytes(7), magic=GNU) + END)
    add("b256_size_2^64", member(b"m", size_field=b"\x80\x00\x00\x01" + bytes(8), magic=GNU) + END)
    add("b256_size_2^63-1", member(b"m", size_field=b"\x80\x00\x00\x00\x7f" + b"\xff" * 7, magic=GNU) + END)  # legal: "truncated member"
    # a negative base-256 mode (all ones was taken as 07777): REFUSED, not masked
    add("b256_mode_all_ones", member(b"m", b"1", mode_field=b"\xff" * 8, magic=GNU) + END)
    for typ in (b"L", b"K", b"x"):
        add("%s_size_exceeds_stream" % typ.decode(), header(b"meta", typ, size=4096) + pad(b"13 path=abcd\n") + member(b"m") + END)
        add("%s_size_eleven_7s" % typ.decode(), header(b"meta", typ, size_field=b"77777777777\x00") + member(b"m") + END)
    # an 'L' with no member behind it: refused, as tarfile does ("missing or bad subsequent header"); archive/tar ends quietly
    add("L_at_the_very_end", member(b"ok", b"1") + gnu_long(b"L", b"name-of-nothing"))
    add("L_before_the_zero_blocks", member(b"ok", b"1") + gnu_long(b"L", b"name-of-nothing") + END)
    add("x_at_the_very_end", member(b"ok", b"1") + pax(ok13))
    add("zero_block_then_a_header", member(b"ok", b"1") + bytes(512) + member(b"late", b"2") + END)
    # member types UnpackTar does not create
    for typ in (b"1", b"3", b"4", b"6", b"S", b"g", b"M"):
        body = pad(b"13 path=abcd\n") if typ == b"g" else b""
        add("type_" + typ.decode(), member(b"ok", b"1") + header(b"t", typ, size=13 if body else 0, link=b"ok") + body + END, ECONTENT)
    # ".." anywhere in the cleaned name
    add("dotdot_via_prefix", member(b"x", b"1", prefix=b"..") + END, ECONTENT)
    add("dotdot_via_L", gnu_long(b"L", b"../x") + member(b"s", b"1") + END, ECONTENT)
    add("dotdot_via_pax_path", pax(record(b"path", b"a/../../x")) + member(b"s", b"1") + END, ECONTENT)
    add("dotdot_plain", member(b"../x", b"1") + END, ECONTENT)
    add("a..b", member(b"a..b", b"1") + END, ECONTENT)
    return cases


def clean_table():
    """A few hundred generated paths with what filepath.Clean makes of each: posixpath.normpath where the two agree (no
    leading "//", not empty), else by hand."""
    parts = [b"", b".", b"..", b"a", b"bc", b"..."]
    paths = set()
    for lead in (b"", b"/", b"./", b"../"):
        for a in parts:
            for b in parts:
                for c in parts:
                    for trail in (b"", b"/"):
                        paths.add(lead + b"/".join((a, b, c)) + trail)
    table = []
    for p in sorted(paths):
        if p.startswith(b"//") or not p:
            continue
        table.append((p, posixpath.normpath(p)))
    # BY HAND: where normpath and Clean differ
    table += [(b"", b"."), (b"//", b"/"), (b"//a", b"/a"), (b"//a//b/", b"/a/b"), (b"///a", b"/a"), (b"//..", b"/"),
              (b"../..", b"../.."), (b"../a/../..", b"../.."), (b"a/../..", b".."), (b"/..", b"/"), (b"/../a", b"/a")]
    return table
