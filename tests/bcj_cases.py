"""Inputs for the .xz BCJ filters (x86, ARM, ARM-Thumb: snappy_amd/csrc/bcj_core.h, bcj_kernels.hip) and their oracle,
liblzma through Python's lzma.  A filter alone cannot be asked of liblzma, so the oracle goes through raw LZMA2:
  encode: compress raw with [BCJ, LZMA2], decompress raw with [LZMA2]      -> the filtered bytes
  decode: compress raw with [LZMA2],      decompress raw with [BCJ, LZMA2] -> the bytes with the filter undone
Shared by tests/test_bcj_host.py (the host code, the kernels' cut run stretch by stretch) and the GPU tests
(tests/test_gpu_bcj_edges.py, tests/test_gpu_xz_bcj.py).  Also: .xz files whose Blocks carry different filter chains,
assembled from xz_cases.py's parts, and headers liblzma refuses."""
import functools
import lzma
import random
import struct
import zlib

import xz_cases as X

X86, ARM, THUMB = 4, 7, 8
FILTERS = (X86, ARM, THUMB)
NAMES = {X86: "x86", ARM: "arm", THUMB: "armthumb"}
LZMA_ID = {X86: lzma.FILTER_X86, ARM: lzma.FILTER_ARM, THUMB: lzma.FILTER_ARMTHUMB}
STRETCH = 256  # kBcjStretch: the bytes a lane owns in the kernels
TILE = 65536   # a workgroup's 256 stretches
STARTS = (0, 4096, 0xFFFFFFF0)  # multiples of every filter's alignment; the last wraps positions around 2^32
_LZ = dict(id=lzma.FILTER_LZMA2, preset=0)


def _bcj(filt, start):
    f = dict(id=LZMA_ID[filt])
    if start:
        f["start_offset"] = start
    return f


def oracle(filt, encode, data, start=0):
    """liblzma's bytes for `data` as one Block through the filter."""
    data = bytes(data)
    if encode:
        return lzma.decompress(lzma.compress(data, format=lzma.FORMAT_RAW, filters=[_bcj(filt, start), _LZ]), format=lzma.FORMAT_RAW, filters=[_LZ])
    return lzma.decompress(lzma.compress(data, format=lzma.FORMAT_RAW, filters=[_LZ]), format=lzma.FORMAT_RAW, filters=[_bcj(filt, start), _LZ])


# ---- data ------------------------------------------------------------------------------------------------------------

def drawn(n, alphabet, seed):
    r = random.Random(seed)
    return bytes(r.choice(alphabet) for _ in range(n))


def x86_dense(n, seed):
    """bytes drawn from {E8, E9, 00, FF, 12}: opcode bytes everywhere, and high bytes that make them candidates"""
    return drawn(n, (0xE8, 0xE9, 0x00, 0xFF, 0x12), seed)


def x86_code(n, seed):
    """something like machine code: calls of a few functions from many places, between other bytes"""
    r = random.Random(seed)
    targets = [r.randrange(0, max(n, 1)) for _ in range(6)]
    out = bytearray()
    while len(out) < n:
        out += bytes(r.randrange(256) for _ in range(r.randrange(1, 24)))
        rel = (r.choice(targets) - (len(out) + 5)) & 0xFFFFFFFF
        out += bytes([r.choice((0xE8, 0xE9))]) + struct.pack("<I", rel)
    return bytes(out[:n])


def x86_mask_states():
    """A candidate behind each of the eight patterns of opcode bytes in its three bytes in front (prev_mask's states), with
    both high bytes, and offsets whose sum with the position carries into (or borrows from) the high byte: 00 <-> FF."""
    r = random.Random(71)
    out = bytearray()
    for mask in range(8):
        for high in (0x00, 0xFF):
            for mid in ((0xFF, 0xFF, 0xFF), (0x00, 0x00, 0x00), (0xF0, 0xFF, 0xFF), (0x10, 0x00, 0x00), (0x34, 0x00, 0xFF), (0x56, 0xFF, 0x00),
                        (r.randrange(256), r.randrange(256), r.randrange(256))):
                out += bytes(6)  # a restart point between the cases
                out += bytes(0xE8 if mask & (4 >> k) else 0x12 for k in range(3))
                out += bytes([r.choice((0xE8, 0xE9))]) + bytes(mid) + bytes([high])
                out += bytes([r.choice((0x00, 0xFF, 0xE8, 0x12)) for _ in range(3)])
    return bytes(out)


def arm_code(n, seed):
    r = random.Random(seed)
    out = bytearray(r.randrange(256) for _ in range(n))
    for i in range(0, n - 3, 4):
        k = r.randrange(4)
        if k == 0:
            out[i + 3] = 0xEB  # BL
        elif k == 1:
            out[i + r.randrange(3)] = 0xEB  # the byte where it does not count
    return bytes(out)


def thumb_code(n, seed):
    r = random.Random(seed)
    out = bytearray(r.randrange(256) for _ in range(n))
    for i in range(0, n - 3, 2):
        k = r.randrange(5)
        if k == 0:
            out[i + 1] = 0xF0 | r.randrange(8)
            out[i + 3] = 0xF8 | r.randrange(8)
        elif k == 1:
            out[i + 1] = 0xF0 | r.randrange(8)  # half a candidate
        elif k == 2:
            out[i + 1] = 0xF8 | r.randrange(8)
    return bytes(out)


def code(filt, n, seed):
    return {X86: x86_code, ARM: arm_code, THUMB: thumb_code}[filt](n, seed)


def _candidate(filt):
    """one convertible instruction of the filter"""
    return {X86: b"\xE8\x10\x20\x30\x00", ARM: b"\x10\x20\x30\xEB", THUMB: b"\x10\xF1\x20\xF9"}[filt]


@functools.lru_cache(maxsize=None)
def filter_cases(filt):
    """[(name, data, start_offset)] for one filter: every length and tail the issue of the filters' edges names."""
    out = []
    dense = {X86: x86_dense, ARM: lambda n, s: drawn(n, (0xEB, 0x00, 0xFF, 0x12), s), THUMB: lambda n, s: drawn(n, (0xF0, 0xF7, 0xF8, 0xFF, 0x12), s)}[filt]
    for n in list(range(10)) + [63, 64, 65, STRETCH - 1, STRETCH, STRETCH + 1, 3 * STRETCH + 5]:
        out.append(("dense_%d" % n, dense(n, 100 + n), 0))
        out.append(("code_%d" % n, code(filt, n, 200 + n), 0))
    cand = _candidate(filt)
    for back in (4, 5, 6):  # a candidate that begins `back` bytes before the end, at an aligned place and at an odd one
        for front in (64, 65, 66, 67):
            d = (bytes(front) + cand + bytes(8))[:front + back]
            out.append(("tail_%d_front_%d" % (back, front), d, 0))
    for start in STARTS:
        out.append(("code_start_%x" % start, code(filt, 5000, 300 + start % 97), start))
        out.append(("dense_start_%x" % start, dense(3000, 400 + start % 97), start))
    if filt == X86:
        out.append(("mask_states", x86_mask_states(), 0))
        out.append(("mask_states_start", x86_mask_states(), 0xFFFFFFF0))
        out.append(("e8_run_three_stretches", bytes(7) + b"\xE8" * (3 * STRETCH + 9) + x86_code(600, 5), 0))
        out.append(("e8_e9_run_then_candidates", b"\xE9\xE8" * 300 + b"\x00" * 4 + x86_dense(900, 6), 0))
        out.append(("e8_run_whole_tile", x86_code(100, 7) + b"\xE8" * (TILE + 2 * STRETCH) + x86_code(1000, 8), 0))
        out.append(("zeros_and_calls", (bytes(5) + b"\xE8\x00\x00\x00\x00") * 300, 0))
    out.append(("code_70000", code(filt, 70000, 9), 4096))
    return out


def all_cases():
    return [(f, name, data, start) for f in FILTERS for name, data, start in filter_cases(f)]


# ---- .xz files ---------------------------------------------------------------------------------------------------------

def filter_flags(filt, props=b""):
    """a BCJ filter's entry in a Block header: id, size of properties, properties"""
    return X.vli(filt) + X.vli(len(props)) + props


def block_header(chain, dict_size, csize=None, usize=None):
    """xz_cases.block_header with a filter chain in front of LZMA2: chain = [filter flags, ...]"""
    flags = (0x40 if csize is not None else 0) | (0x80 if usize is not None else 0) | len(chain)
    body = b""
    if csize is not None:
        body += X.vli(csize)
    if usize is not None:
        body += X.vli(usize)
    body += b"".join(chain) + b"\x21\x01" + bytes([X.dict_byte(dict_size)])
    n = (2 + len(body) + 4 + 3) & ~3
    h = bytes([n // 4 - 1, flags]) + body
    h += bytes(n - 4 - len(h))
    return h + struct.pack("<I", zlib.crc32(h))


def xz_chained(blocks, check=X.CHECK_CRC64, check_over_filtered=False):
    """One Stream.  blocks: [(data, chain)], chain = [] or [(filter id, properties bytes)]: the Block's LZMA2 data is made
    by liblzma from the data filtered by this module's oracle.  check_over_filtered: the Check field taken over the filtered
    bytes, which the format does not allow."""
    flags = bytes([0, check])
    d = bytearray(X.MAGIC + flags + struct.pack("<I", zlib.crc32(flags)))
    recs = []
    for data, chain in blocks:
        filtered = data
        for fid, props in chain:
            start = struct.unpack("<I", props)[0] if len(props) == 4 else 0
            if fid in FILTERS and start % {X86: 1, ARM: 4, THUMB: 2}[fid] == 0:  # (a start_offset liblzma refuses: the data stays as it is)
                filtered = oracle(fid, True, filtered, start)
        raw = lzma.compress(filtered, format=lzma.FORMAT_RAW, filters=[dict(id=lzma.FILTER_LZMA2, preset=0, dict_size=1 << 20)])
        h = block_header([filter_flags(fid, props) for fid, props in chain], 1 << 20, len(raw), len(data))
        ck = X.check_field(check, filtered if check_over_filtered else data)
        recs.append((len(h) + len(raw) + len(ck), len(data)))
        d += h + raw + bytes(-(len(h) + len(raw)) % 4) + ck
    ix = X.index_field(recs)
    d += ix
    tail = struct.pack("<I", len(ix) // 4 - 1) + flags
    d += struct.pack("<I", zlib.crc32(tail)) + tail + b"YZ"
    return bytes(d)


def liblzma_file(filt, data, start=0, check=lzma.CHECK_CRC64):
    return lzma.compress(data, format=lzma.FORMAT_XZ, check=check, filters=[_bcj(filt, start), dict(id=lzma.FILTER_LZMA2, preset=1)])


@functools.lru_cache(maxsize=None)
def good_files():
    """[(name, file, plain)]: files liblzma reads, every Block one LZMA2 or one BCJ filter in front of one LZMA2"""
    out = []
    for f in FILTERS:
        plain = code(f, 150000, 20 + f)
        out.append(("liblzma_" + NAMES[f], liblzma_file(f, plain), plain))
        out.append(("liblzma_%s_start" % NAMES[f], liblzma_file(f, plain[:30000], 4096, lzma.CHECK_SHA256), plain[:30000]))
    parts = [(code(X86, 65536, 31), [(X86, b"")]), (code(ARM, 65536, 32), [(ARM, b"")]), (X.text(65536, 33), []),
             (code(THUMB, 65536, 34), [(THUMB, struct.pack("<I", 0x1000))]), (code(X86, 1234, 35), [(X86, struct.pack("<I", 0xFFFFFFF0))]),
             (b"", [(X86, b"")]), (code(ARM, 7, 36), [(ARM, struct.pack("<I", 8))])]
    for check in (X.CHECK_CRC64, X.CHECK_CRC32, X.CHECK_SHA256, X.CHECK_NONE):
        out.append(("mixed_chains_check_%d" % check, xz_chained(parts, check), b"".join(p[0] for p in parts)))
    for name, z, plain in out:
        assert X.ref_decompress(z) == plain, name
    return out


@functools.lru_cache(maxsize=None)
def other_chain_files():
    """[(name, file, text)]: chains that stay SNAPHASH_EINVAL with and without SNAPHASH_UNXZ_BCJ, and the text that names
    the first filter that is not LZMA2"""
    t = X.text(20000, 40)
    lz = dict(id=lzma.FILTER_LZMA2, preset=0)
    out = [("delta", lzma.compress(t, format=lzma.FORMAT_XZ, filters=[dict(id=lzma.FILTER_DELTA, dist=4), lz]), "xz: unsupported filter 0x03"),
           ("two_bcj", lzma.compress(t, format=lzma.FORMAT_XZ, filters=[dict(id=lzma.FILTER_X86), dict(id=lzma.FILTER_ARM), lz]), "xz: unsupported filter 0x04"),
           ("powerpc", lzma.compress(t, format=lzma.FORMAT_XZ, filters=[dict(id=lzma.FILTER_POWERPC), lz]), "xz: unsupported filter 0x05"),
           ("ia64", lzma.compress(t, format=lzma.FORMAT_XZ, filters=[dict(id=lzma.FILTER_IA64), lz]), "xz: unsupported filter 0x06"),
           ("sparc", lzma.compress(t, format=lzma.FORMAT_XZ, filters=[dict(id=lzma.FILTER_SPARC), lz]), "xz: unsupported filter 0x09"),
           ("delta_then_x86", lzma.compress(t, format=lzma.FORMAT_XZ, filters=[dict(id=lzma.FILTER_DELTA, dist=1), dict(id=lzma.FILTER_X86), lz]),
            "xz: unsupported filter 0x03"),
           ("unknown_id_0x0b", xz_chained([(t, [(0x0B, b"")])]), "xz: unsupported filter 0x0B")]
    for name, z, _ in out[:-1]:
        assert lzma.decompress(z) == t, name
    return out


@functools.lru_cache(maxsize=None)
def refused_files():
    """[(name, file)]: a BCJ chain liblzma refuses by its properties: SNAPHASH_EFORMAT with the flag, the plain entries'
    SNAPHASH_EINVAL without"""
    t = code(X86, 5000, 50)
    out = [("props_1_byte", xz_chained([(t, [(X86, b"\x00")])])), ("props_5_bytes", xz_chained([(t, [(X86, bytes(5))])])),
           ("arm_start_2", xz_chained([(t, [(ARM, struct.pack("<I", 2))])])), ("thumb_start_1", xz_chained([(t, [(THUMB, struct.pack("<I", 1))])]))]
    for name, z in out:
        assert X.refuses(lzma.decompress, z), name
    return out


def check_over_filtered_file():
    """A Block whose Check was taken over the filtered bytes; the data is such that the filter changes it."""
    t = code(X86, 40000, 60)
    assert oracle(X86, True, t) != t
    z = xz_chained([(t, [(X86, b"")])], check_over_filtered=True)
    assert X.refuses(lzma.decompress, z)
    return z
