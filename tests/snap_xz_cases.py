"""The .xz members of the container tests (tests/test_gpu_snap_xz.py), beside tests/snap_cases.py, whose tree, tar and ar
writer they use: every form of a data.tar.xz / control.tar.xz the session must read, written by Python's lzma -- or, for
the two "own" forms, by the library's producer -- and the places of a .xz file a test flips a byte in.  A builder, not a
test."""
import lzma
import struct

import snap_cases as S

BLOCK = 65536  # the own forms' Block size: the tree's tar stream is more than one of them

LZMA2 = {"id": lzma.FILTER_LZMA2, "preset": 6}
PY_FORMS = {
    "xz1": dict(),                                   # one Block, CRC-64: what `xz --compress --stdout` writes
    "xzsha": dict(check=lzma.CHECK_SHA256),
    "xzcrc32": dict(check=lzma.CHECK_CRC32),
    "xznone": dict(check=lzma.CHECK_NONE),
    "xzx86": dict(filters=[{"id": lzma.FILTER_X86}, LZMA2]),
}
OWN_FORMS = {"own": dict(), "own-x86-L1": dict(filter="x86", level=1)}
FORMS = list(PY_FORMS) + ["xzcat"] + list(OWN_FORMS)


def xz(data, **kw):
    return lzma.compress(data, format=lzma.FORMAT_XZ, **kw)


def compress(form, tar, ctx=None):
    """The bytes of the .xz member of a form (ctx: for the own forms)."""
    if form in PY_FORMS:
        return xz(tar, **PY_FORMS[form])
    if form == "xzcat":  # two Streams, Stream Padding (a multiple of four zero bytes) between them
        cut = (len(tar) // 2) & ~511
        return xz(tar[:cut]) + b"\0" * 8 + xz(tar[cut:], check=lzma.CHECK_CRC32)
    return ctx.xz_buffer(tar, block_size=BLOCK, **OWN_FORMS[form])


def delta(tar):
    """A chain the session does not take: Delta in front of LZMA2."""
    return xz(tar, filters=[{"id": lzma.FILTER_DELTA, "dist": 4}, LZMA2])


def control_tar(yaml, manifest=b"{}\n"):
    ents = [("./manifest", manifest)]
    if yaml is not None:
        ents.insert(0, ("./hashes.yaml", yaml))
    return S.tar_files(ents)


def write_snap(path, control, data):
    """debian-binary, then the two members as (name, bytes), control first as snaphash_snap_build and dpkg-deb lay them out."""
    with open(path, "wb") as f:
        f.write(S.ar_pack([("debian-binary", b"2.0\n"), control, data]))


def layout(blob):
    """Where things are in a one-Stream .xz file: {"body": an offset inside the first Block's compressed data, "check": the
    last byte of the last Block's Check field, "index": a byte of the Index's first record}.  From the format: a 12-byte
    Stream Header; a Block Header of (first byte + 1) * 4 bytes; at the end a 12-byte Stream Footer whose Backward Size says
    how long the Index in front of it is, and in front of the Index the last Block's Check."""
    assert blob[:6] == b"\xfd7zXZ\0" and blob[-2:] == b"YZ"
    index_size = (struct.unpack("<I", blob[-8:-4])[0] + 1) * 4
    index = len(blob) - 12 - index_size
    assert blob[index] == 0  # the Index Indicator
    header = (blob[12] + 1) * 4
    check_size = {0: 0, 1: 4, 4: 8, 10: 32}[blob[7] & 15]
    assert check_size, "a file without a Check has no Check field to flip"
    return {"body": 12 + header + 300, "check": index - 1, "index": index + 2}


def flip(blob, at):
    return blob[:at] + bytes([blob[at] ^ 0x10]) + blob[at + 1:]
