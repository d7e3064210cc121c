"""Inputs for the .xz filters beyond x86 / ARM / ARM-Thumb -- PowerPC, IA64, SPARC (snappy_amd/csrc/bcj_core.h) and Delta
(delta_core.h, delta_kernels.hip) -- and their oracle, liblzma through Python's lzma, the way tests/bcj_cases.py asks it:
  encode: compress raw with [F, LZMA2], decompress raw with [LZMA2]      -> the filtered bytes
  decode: compress raw with [LZMA2],    decompress raw with [F, LZMA2]   -> the bytes with the filter undone
Shared by tests/test_xzfilt_host.py (the host code and the kernels' pieces run lane by lane) and
tests/test_gpu_xzfilt_edges.py (the kernels).  An oracle answer is computed once a process and handed out unchanged."""
import functools
import lzma
import random

import xz_cases as X

DELTA, X86, POWERPC, IA64, ARM, THUMB, SPARC = 3, 4, 5, 6, 7, 8, 9
WORD_FILTERS = (POWERPC, IA64, SPARC)  # the ones new here; a lane a word (IA64: a 16-byte bundle)
NAMES = {DELTA: "delta", X86: "x86", POWERPC: "powerpc", IA64: "ia64", ARM: "arm", THUMB: "armthumb", SPARC: "sparc"}
LZMA_ID = {DELTA: lzma.FILTER_DELTA, X86: lzma.FILTER_X86, POWERPC: lzma.FILTER_POWERPC, IA64: lzma.FILTER_IA64, ARM: lzma.FILTER_ARM,
           THUMB: lzma.FILTER_ARMTHUMB, SPARC: lzma.FILTER_SPARC}
UNIT = {POWERPC: 4, IA64: 16, SPARC: 4}  # the filter's unit and the alignment of its start_offset
STRETCH = 256  # kBcjStretch
TILE = 65536   # kDeltaTile, and a workgroup's 256 stretches
STARTS = (0, 4096, 0xFFFFFFF0)  # multiples of 16; the last wraps positions around 2^32
_LZ = dict(id=lzma.FILTER_LZMA2, preset=0)


def lzma_filter(filt, param=0):
    """liblzma's filter entry: param is Delta's distance, a BCJ filter's start_offset"""
    if filt == DELTA:
        return dict(id=lzma.FILTER_DELTA, dist=param)
    f = dict(id=LZMA_ID[filt])
    if param:
        f["start_offset"] = param
    return f


@functools.lru_cache(maxsize=None)
def oracle(filt, encode, data, param=0):
    """liblzma's bytes for `data` as one Block through the filter"""
    data = bytes(data)
    f = lzma_filter(filt, param)
    if encode:
        return lzma.decompress(lzma.compress(data, format=lzma.FORMAT_RAW, filters=[f, _LZ]), format=lzma.FORMAT_RAW, filters=[_LZ])
    return lzma.decompress(lzma.compress(data, format=lzma.FORMAT_RAW, filters=[_LZ]), format=lzma.FORMAT_RAW, filters=[f, _LZ])


# ---- the word filters' data ------------------------------------------------------------------------------------------------

def rnd(n, seed):
    return random.Random(seed).randbytes(n)


def drawn(n, alphabet, seed):
    r = random.Random(seed)
    return bytes(r.choices(alphabet, k=n))


def ia64_bundle(r, templ, hits=(True, True, True)):
    """One bundle of the template whose slot s is a candidate (opcode 5 in bits 37 .. 40, bits 9 .. 11 clear) where hits[s];
    every other bit random -- the 21 address bits among them."""
    v = templ & 0x1F
    for s in range(3):
        n = r.getrandbits(41)
        if hits[s]:
            n = (n & ~(0xF << 37) & ~(7 << 9)) | (5 << 37)
        v |= n << (5 + 41 * s)
    return v.to_bytes(16, "little")


def candidate(filt, r=None):
    """one convertible unit of the filter"""
    r = r or random.Random(1)
    if filt == POWERPC:
        return bytes([0x48 | r.randrange(4), r.randrange(256), r.randrange(256), (r.randrange(64) << 2) | 1])
    if filt == SPARC:
        if r.randrange(2):
            return bytes([0x40, r.randrange(0x40), r.randrange(256), r.randrange(256)])
        return bytes([0x7F, 0xC0 | r.randrange(0x40), r.randrange(256), r.randrange(256)])
    return ia64_bundle(r, 0x16)  # a template whose three slots may all branch


def code(filt, n, seed):
    """something like code: candidates at one unit in three, near misses at another, random bytes between"""
    r = random.Random(seed)
    u = UNIT[filt]
    out = bytearray(r.randbytes(n))
    for i in range(0, n - u + 1, u):
        k = r.randrange(3)
        if k == 0:
            out[i:i + u] = candidate(filt, r)
        elif k == 1:  # a candidate with one deciding bit wrong
            c = bytearray(candidate(filt, r))
            if filt == POWERPC:
                c[3] ^= r.choice((1, 2))
            elif filt == SPARC:
                c[1] ^= 0x80
            else:
                c[0] = (c[0] & 0xE0) | r.choice((0x00, 0x14, 0x1A))  # a template without branch slots
            out[i:i + u] = c
    return bytes(out)


def dense(filt, n, seed):
    """bytes from an alphabet that makes candidates out of random draws (IA64: bundles of every template, all slots hit)"""
    if filt == POWERPC:
        return drawn(n, (0x48, 0x4B, 0x01, 0xFD, 0xFF, 0x00), seed)
    if filt == SPARC:
        return drawn(n, (0x40, 0x7F, 0x00, 0x3F, 0xC0, 0xFF), seed)
    r = random.Random(seed)
    return b"".join(ia64_bundle(r, r.randrange(32)) for _ in range(n // 16 + 1))[:n]


LENGTHS = (0, 1, 3, 4, 15, 16, 17, 255, 256, 257, TILE + 5)


@functools.lru_cache(maxsize=None)
def word_cases(filt):
    """[(name, data, start_offset)] for one of the three word filters"""
    u = UNIT[filt]
    out = []
    for n in LENGTHS:
        out.append(("dense_%d" % n, dense(filt, n, 100 + n), 0))
        out.append(("code_%d" % n, code(filt, n, 200 + n), 0))
    r = random.Random(7)
    cand = candidate(filt, r)
    for front in (0, u, STRETCH - u, STRETCH, 3 * STRETCH):
        out.append(("last_unit_front_%d" % front, bytes(front) + cand, 0))                      # the Block's last unit: converted
        out.append(("cut_unit_front_%d" % front, bytes(front) + cand[:-1], 0))                  # one byte short: left alone
        out.append(("partial_behind_front_%d" % front, bytes(front) + cand + cand[:u - 1], 0))  # a whole one, then a partial one
    for start in STARTS:
        out.append(("code_start_%x" % start, code(filt, 5000, 300 + start % 97), start))
        out.append(("dense_start_%x" % start, dense(filt, 3000, 400 + start % 97), start))
    if filt == IA64:  # every template, all three slots candidates, at positions that count
        for start in STARTS:
            out.append(("every_template_start_%x" % start, b"".join(ia64_bundle(r, t) for t in range(32) for _ in range(3)), start))
        out.append(("slots_one_at_a_time", b"".join(ia64_bundle(r, 0x16, tuple(s == k for s in range(3))) for k in range(3) for _ in range(8)), 4096))
    if filt == SPARC:  # both sign forms, with displacements whose sum with the position crosses bit 22 in both directions
        words = [bytes([0x40, 0x3F, 0xFF, 0xFF]), bytes([0x40, 0x00, 0x00, 0x00]), bytes([0x7F, 0xC0, 0x00, 0x00]), bytes([0x7F, 0xFF, 0xFF, 0xFF]),
                 bytes([0x40, 0x1F, 0xFF, 0xFE]), bytes([0x7F, 0xE0, 0x00, 0x01])]
        for start in STARTS:
            out.append(("sign_forms_start_%x" % start, b"".join(words) * 20, start))
    if filt == POWERPC:  # targets that wrap 2^26: the largest offset plus a position, the smallest minus one
        words = [bytes([0x4B, 0xFF, 0xFF, 0xFD]), bytes([0x48, 0x00, 0x00, 0x01]), bytes([0x4B, 0xFF, 0xFF, 0xF1]), bytes([0x48, 0x00, 0x00, 0x0F]),
                 bytes([0x49, 0xFF, 0xFF, 0xFD]), bytes([0x4A, 0x00, 0x00, 0x03])]
        for start in STARTS:
            out.append(("wrap_2_26_start_%x" % start, b"".join(words) * 20, start))
    return out


def all_word_cases():
    return [(f, name, data, start) for f in WORD_FILTERS for name, data, start in word_cases(f)]


# ---- Delta's data ----------------------------------------------------------------------------------------------------------
#
# Why all-0x01 with d = 3 and d = 255 stands beside the random bytes: a decoder that loses a tile's carry goes unseen on any
# input whose column sums over a tile are 0 modulo 256.  Equal bytes x with a d that divides the tile -- d = 1, 2, 4, 16, 256 --
# are such an input: a column holds 65 536 / d of them, and x * 65 536 / d is a multiple of 256 for every one of these d.  With
# d = 3 a tile's columns hold 21 845 or 21 846 ones (85 or 86 modulo 256) and with d = 255 they hold 257 or 258 (1 or 2): the
# carries are nonzero, differ from column to column, and -- 65 536 being no multiple of 3 or 255 -- belong to a column whose
# place in the tile moves from tile to tile.  Random bytes have nonzero carries too, but say nothing by their look when one is lost.

DISTS = (1, 2, 3, 4, 16, 255, 256)


def delta_lengths(d):
    return sorted({0, 1, d - 1, d, d + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + d + 1})


@functools.lru_cache(maxsize=None)
def delta_cases():
    """[(name, data, distance)]"""
    out = []
    for d in DISTS:
        for n in delta_lengths(d):
            out.append(("random_d%d_%d" % (d, n), rnd(n, 1000 * d + n % 977), d))
    for d in (3, 255):
        for n in (TILE + 1, 3 * TILE + d + 1):
            out.append(("ones_d%d_%d" % (d, n), b"\x01" * n, d))
    return out


def three_tile_delta_cases():
    """the cases of more than two tiles: carries cross workgroups"""
    return [(name, data, d) for name, data, d in delta_cases() if len(data) > 2 * TILE]


# ---- .xz files with hand-built Block headers ----------------------------------------------------------------------------------
#
# A file is one Stream of Blocks, each with its own filter list as the header names it: [(id, properties bytes), ...], LZMA2
# (0x21) included wherever the case wants it.  The Block's data is liblzma's raw LZMA2 of the bytes filtered by this module's
# oracle, the header's first filter first; a filter whose properties liblzma refuses leaves the bytes as they are (the file
# is refused anyway).  Every verdict the tests hold is lzma.decompress's of the same file.

LZMA2 = 0x21
PRE_FILTERS = (DELTA, X86, POWERPC, IA64, ARM, THUMB, SPARC)
ALIGN = {X86: 1, POWERPC: 4, IA64: 16, ARM: 4, THUMB: 2, SPARC: 4}
DICT = 1 << 20


def props(filt, param=0):
    """the properties liblzma writes: Delta's distance less one; a BCJ filter's start_offset, or nothing for 0"""
    import struct
    if filt == LZMA2:
        return bytes([X.dict_byte(DICT)])
    if filt == DELTA:
        return bytes([param - 1])
    return struct.pack("<I", param) if param else b""


def chain_of(*filters):
    """[(id, properties)] with LZMA2 behind: a filter is an id, or (id, param)"""
    out = [(f[0], props(*f)) if isinstance(f, tuple) else (f, props(f, 1 if f == DELTA else 0)) for f in filters]
    return out + [(LZMA2, props(LZMA2))]


def block_header(filters, csize, usize):
    import struct
    import zlib
    body = X.vli(csize) + X.vli(usize) + b"".join(X.vli(fid) + X.vli(len(p)) + p for fid, p in filters)
    n = (2 + len(body) + 4 + 3) & ~3
    h = bytes([n // 4 - 1, 0xC0 | (len(filters) - 1)]) + body
    h += bytes(n - 4 - len(h))
    return h + struct.pack("<I", zlib.crc32(h))


def filtered(data, filters):
    import struct
    for fid, p in filters:
        if fid == DELTA and len(p) == 1:
            data = oracle(DELTA, True, data, p[0] + 1)
        elif fid in ALIGN and len(p) in (0, 4):
            start = struct.unpack("<I", p)[0] if p else 0
            if start % ALIGN[fid] == 0:
                data = oracle(fid, True, data, start)
    return data


def xz_stream(blocks, check=None):
    """One Stream.  blocks: [(data, filters)]"""
    import struct
    import zlib
    check = X.CHECK_CRC64 if check is None else check
    flags = bytes([0, check])
    d = bytearray(X.MAGIC + flags + struct.pack("<I", zlib.crc32(flags)))
    recs = []
    for data, filters in blocks:
        raw = lzma.compress(filtered(data, filters), format=lzma.FORMAT_RAW, filters=[dict(id=lzma.FILTER_LZMA2, preset=0, dict_size=DICT)])
        h = block_header(filters, len(raw), len(data))
        ck = X.check_field(check, data)
        recs.append((len(h) + len(raw) + len(ck), len(data)))
        d += h + raw + bytes(-(len(h) + len(raw)) % 4) + ck
    ix = X.index_field(recs)
    d += ix
    tail = struct.pack("<I", len(ix) // 4 - 1) + flags
    d += struct.pack("<I", zlib.crc32(tail)) + tail + b"YZ"
    return bytes(d)


def mixed(n, seed):
    """bytes with something for every filter: candidates of the six BCJ filters among text and a 16-bit ramp"""
    r = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        k = r.randrange(8)
        if k < 3:
            out += candidate((POWERPC, IA64, SPARC)[k], r)
        elif k == 3:
            out += b"\xE8" + r.randbytes(3) + bytes([r.choice((0, 0xFF))])
        elif k == 4:
            out += r.randbytes(3) + b"\xEB"
        elif k == 5:
            out += bytes([r.randrange(256), 0xF0 | r.randrange(8), r.randrange(256), 0xF8 | r.randrange(8)])
        elif k == 6:
            out += b"".join(((len(out) + 2 * i) & 0xFFFF).to_bytes(2, "little") for i in range(8))
        else:
            out += X.text(r.randrange(1, 40), r.randrange(1 << 20))
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def chain_files():
    """[(name, file, plain or None)]: plain is lzma.decompress's answer, None where liblzma refuses the file"""
    import itertools
    import struct
    data = mixed(1500, 11)
    param = {DELTA: 3, X86: 0, POWERPC: 4096, IA64: 16, ARM: 0, THUMB: 2, SPARC: 4}
    files = []
    for k in (1, 2, 3):  # every permutation (repeats allowed) of one, two and three pre-filters drawn from all seven
        for combo in itertools.product(PRE_FILTERS, repeat=k):
            files.append(("chain_" + "_".join(NAMES[f] for f in combo), xz_stream([(data, chain_of(*((f, param[f]) for f in combo)))])))
    pre = lambda *fs: [(f, props(f, 1 if f == DELTA else 0)) for f in fs]
    lz = (LZMA2, props(LZMA2))
    files += [
        ("four_pre_filters", xz_stream([(data, pre(DELTA, X86, POWERPC, SPARC))])),             # (the header holds four filters at most)
        ("three_pre_filters_no_lzma2", xz_stream([(data, pre(X86, DELTA, ARM))])),
        ("lzma2_first", xz_stream([(data, [lz] + pre(X86) + [lz])])),
        ("lzma2_in_the_middle", xz_stream([(data, pre(DELTA) + [lz] + pre(X86) + [lz])])),
        ("lzma2_not_last", xz_stream([(data, [lz] + pre(X86))])),
        ("delta_props_0_bytes", xz_stream([(data, [(DELTA, b""), lz])])),
        ("delta_props_2_bytes", xz_stream([(data, [(DELTA, b"\x01\x00"), lz])])),
        ("delta_props_2_bytes_behind_x86", xz_stream([(data, pre(X86) + [(DELTA, b"\x01\x00"), lz])])),
        ("delta_dist_256", xz_stream([(data, [(DELTA, b"\xff"), lz])])),
        ("bcj_props_1_byte", xz_stream([(data, [(SPARC, b"\x00"), lz])])),
        ("bcj_props_5_bytes", xz_stream([(data, pre(DELTA) + [(POWERPC, bytes(5)), lz])])),
        ("arm64_0x0a", xz_stream([(data, [(0x0A, b""), lz])])),
        ("riscv_0x0b_behind_delta", xz_stream([(data, pre(DELTA) + [(0x0B, b""), lz])])),
    ]
    for f, a in ALIGN.items():  # each BCJ offset off its alignment, and on it
        for off in sorted({1, a // 2, a + 1, a, 2 * a} - {0}):
            files.append(("%s_offset_%d" % (NAMES[f], off), xz_stream([(data, [(f, struct.pack("<I", off)), lz])])))
    # Blocks and Streams with different chains, an empty Block and an unfiltered one among them
    parts = [(mixed(70000, 12), chain_of((DELTA, 2))), (mixed(3000, 13), chain_of(POWERPC)), (X.text(5000, 14), [lz]), (b"", chain_of(IA64, IA64)),
             (mixed(66000, 15), chain_of((DELTA, 3), X86, SPARC)), (mixed(100, 16), chain_of((IA64, 32), (DELTA, 256), (THUMB, 6)))]
    for check in (X.CHECK_CRC64, X.CHECK_CRC32, X.CHECK_SHA256, X.CHECK_NONE):
        files.append(("mixed_blocks_check_%d" % check, xz_stream(parts, check)))
    files.append(("two_streams", xz_stream(parts[:2]) + bytes(8) + xz_stream(parts[4:], X.CHECK_SHA256)))
    out = []
    for name, z in files:
        try:
            plain = X.ref_decompress(z)
        except (lzma.LZMAError, EOFError):
            plain = None
        out.append((name, z, plain))
    return out


def liblzma_chain_file(data, chain, check=lzma.CHECK_CRC64, preset=1):
    """a file liblzma writes itself.  chain: [id or (id, param)]"""
    fs = [lzma_filter(*f) if isinstance(f, tuple) else lzma_filter(f, 1 if f == DELTA else 0) for f in chain]
    return lzma.compress(data, format=lzma.FORMAT_XZ, check=check, filters=fs + [dict(id=lzma.FILTER_LZMA2, preset=preset)])


# the chains the producer's tests name
PRODUCER_CHAINS = ([(DELTA, 2)], [POWERPC], [(DELTA, 3), X86, SPARC], [IA64, IA64])
