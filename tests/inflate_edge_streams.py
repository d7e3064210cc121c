"""Builders of the gzip streams that put the GPU inflate path (inflate_kernels.hip and its driver in unpack.inc) at its own
edges: plain Python, no GPU, no library.  One function per item of the list in tests/test_inflate_edges_host.py; each
returns a dict with the stream ("gz"), the bytes it decodes to ("data", None where the stream is invalid), the raw
DEFLATE stream of its (last) member ("raw"), and the facts the tests rely on -- the byte offsets in "raw" at which its
flush-terminated segments start ("starts"), their output lengths ("lens"), planted bit offsets.  tests/
test_inflate_edges_host.py checks every stream against zlib and the shape each one claims against the host harnesses;
tests/test_gpu_inflate_edges.py sends them through the kernels."""
import struct
import zlib

import numpy as np

from test_inflate_host import BitWriter, raw_deflate  # noqa: F401  (raw_deflate: re-exported for the tests)

GZ_HEADER = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03"
FINAL_EMPTY_STORED = b"\x01\x00\x00\xff\xff"
WINDOW = 32768
SLOT_SYMS = 65536 + 4096          # inflate_kernels.h kInflateSlotSyms
BLOCK_SLOT_SYMS = 320 << 10       # kInflateBlockSlotSyms
BLOCK_MIN_OUT = 16384             # kInflateBlockMinOut
SPLIT_MIN = 1 << 20               # unpack.inc kSplitMinBytes: a member's first piece in block mode
PIECE_FLOOR = 64 << 10            # the smallest piece staging_bytes can ask for
SCAN_TILE, SCAN_HALO = 4096, 320  # inflate_kernels.hip kScanTile, kScanHalo
HEADER_MAX_BITS = 2286            # inflate_core.h kInfHeaderMaxBits

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
         12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30


def member(raw, data):
    return GZ_HEADER + raw + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def length_symbol(length):
    if length == 258:
        return 285, 0, 0
    i = max(k for k in range(28) if LBASE[k] <= length)
    return 257 + i, LEXT[i], length - LBASE[i]


def distance_symbol(dist):
    i = max(k for k in range(30) if DBASE[k] <= dist)
    return i, DEXT[i], dist - DBASE[i]


def canonical(lens):
    """RFC 1951 sec. 3.2.2: symbol -> (the code's bits in stream order, its length)."""
    top = max(lens)
    count = [0] * (top + 2)
    for l in lens:
        if l:
            count[l] += 1
    nxt, code = [0] * (top + 2), 0
    for l in range(1, top + 1):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (int(format(nxt[l], "0%db" % l)[::-1], 2), l)
            nxt[l] += 1
    return out


def ladder(n, seed):
    """n code lengths of a complete code whose longest codes have 15 bits: the ladder 1, 2, ..., 14, 15, 15 with its
    shortest leaves split until there are n, handed to the symbols in a seeded order."""
    leaves = list(range(1, 16)) + [15]
    while len(leaves) < n:
        l = min(leaves)
        leaves.remove(l)
        leaves += [l + 1, l + 1]
    rng = np.random.default_rng(seed)
    return [int(leaves[i]) for i in rng.permutation(n)]


def dynamic_header(w, final, nlit, ndist, seq, precode=None):
    """A dynamic block's header: seq is the code-length sequence, an int for a length or (16 | 17 | 18, extra bits' value)
    for a repeat; precode: code-length symbol -> its length (default: 0..15 at four bits each, no repeat codes)."""
    if precode is None:
        precode = {s: 4 for s in range(16)}
    w.put(final, 1)
    w.put(2, 2)
    w.put(nlit - 257, 5)
    w.put(ndist - 1, 5)
    ncode = max(4, max(ORDER.index(s) for s in precode) + 1)
    w.put(ncode - 4, 4)
    for s in ORDER[:ncode]:
        w.put(precode.get(s, 0), 3)
    pc = canonical([precode.get(s, 0) for s in range(19)])
    for item in seq:
        sym, extra = item if isinstance(item, tuple) else (item, None)
        w.put(*pc[sym])
        if extra is not None:
            w.put(extra, {16: 2, 17: 3, 18: 7}[sym])


class Stream:
    """A raw DEFLATE stream written block by block, with the bytes it decodes to and the segments (stretches that end
    after a non-final stored block) it consists of."""

    def __init__(self):
        self.w = BitWriter()
        self.out = bytearray()
        self.starts, self.lens, self._seg0 = [0], [], 0
        self.valid = True      # False once a match reaches in front of the stream's first byte
        self.lit_code = self.dist_code = None
        self.lit_lens_used, self.dist_lens_used, self.dists_used = set(), set(), set()

    def _segment_ends(self):
        self.lens.append(len(self.out) - self._seg0)
        self._seg0 = len(self.out)
        self.starts.append(len(self.w.out))

    def stored(self, payload=b"", final=False):
        self.w.put(final, 1)
        self.w.put(0, 2)
        self.w.align()
        self.w.out += struct.pack("<HH", len(payload), len(payload) ^ 0xffff) + payload
        self.out += payload
        if not final:
            self._segment_ends()

    def fixed(self, final=False):
        self.w.put(final, 1)
        self.w.put(1, 2)
        self.lit_code, self.dist_code = canonical(FIXED_LIT), canonical(FIXED_DIST)

    def dynamic(self, lit_lens, dist_lens, final=False):
        dynamic_header(self.w, final, len(lit_lens), len(dist_lens), list(lit_lens) + list(dist_lens))
        self.lit_code, self.dist_code = canonical(lit_lens), canonical(dist_lens)

    def lit(self, byte):
        self.w.put(*self.lit_code[byte])
        self.lit_lens_used.add(self.lit_code[byte][1])
        self.out.append(byte)

    def match(self, length, dist):
        s, eb, ev = length_symbol(length)
        self.w.put(*self.lit_code[s])
        self.lit_lens_used.add(self.lit_code[s][1])
        if eb:
            self.w.put(ev, eb)
        s, eb, ev = distance_symbol(dist)
        self.w.put(*self.dist_code[s])
        self.dist_lens_used.add(self.dist_code[s][1])
        self.dists_used.add(dist)
        if eb:
            self.w.put(ev, eb)
        if dist > len(self.out):
            self.valid = False
            self.out += bytes(length)
        elif dist >= length:
            self.out += self.out[len(self.out) - dist:len(self.out) - dist + length]
        else:
            self.out += (bytes(self.out[-dist:]) * (length // dist + 1))[:length]

    def end_block(self):
        self.w.put(*self.lit_code[256])
        self.lit_lens_used.add(self.lit_code[256][1])

    def finish(self, marker=True):
        """The end of the stream: a final empty stored block (its 00 00 FF FF is a flush candidate, so a piece that
        starts at the last segment still has one ahead and goes through the kernel), or nothing if the caller wrote the
        final block itself."""
        if marker:
            self.stored(b"", final=True)
        self.lens.append(len(self.out) - self._seg0)
        return bytes(self.w.out)

    def result(self, raw, **facts):
        data = bytes(self.out) if self.valid else None
        return dict(gz=member(raw, bytes(self.out)), data=data, raw=raw, starts=self.starts[:len(self.lens)], lens=self.lens, **facts)


def noise(n, seed, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, size=n, dtype=np.uint8).tobytes()


def text(n, seed):
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, size=int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(1500)]
    return b" ".join(words[int(i)] for i in rng.zipf(1.3, size=n // 3 + 8) % 1500)[:n]


def flush_candidates(buf):
    """inflate_host.cpp flush_candidates (the rule of inflate_scan_kernel), restated: sorted byte offsets."""
    a = np.frombuffer(buf, np.uint8).astype(np.int64)
    if len(a) < 4:
        return []
    ln, nl = a[:-3] | a[1:-2] << 8, a[2:-1] | a[3:] << 8
    prev = np.concatenate(([255], a[:-4]))
    j = np.flatnonzero((ln == (~nl & 0xffff)) & ((ln == 0) | (prev < 32)))
    c = j + 4 + ln[j]
    return sorted(set(int(v) for v in c[c <= len(a)]))


def plan_flush(z, starts, lens, piece, cap=SLOT_SYMS):
    """The linking rule of gunzip_engine (unpack.inc) for a member z (raw DEFLATE + trailer) whose true segments start
    at `starts` (byte offsets) and produce `lens` symbols, taken in pieces of `piece` compressed bytes: a piece's chain
    runs from its first byte through the segments that end inside it and fit a slot; where the first one does not, the
    host decodes that segment.  Holds while a piece's candidates fit its slots (64 at least), which the builders see to.
    -> (segments linked into chains, output bytes the host decoder produced)."""
    ends = list(starts[1:]) + [None]
    i, linked, host = 0, 0, 0
    while i < len(starts):
        cur = starts[i]
        pn = min(piece, len(z) - cur)
        cand = set(flush_candidates(z[cur:cur + pn])) | {0}
        nl = 0
        if not (len(cand) == 1 and pn == len(z) - cur):
            while i + nl < len(starts):
                k = i + nl
                if starts[k] - cur not in cand or lens[k] > cap:
                    break
                if ends[k] is None:  # the final segment: it ends with the final block, in front of the trailer
                    if len(z) - 8 - cur > pn:
                        break
                    nl += 1
                    break
                if ends[k] - cur > pn:
                    break
                nl += 1
                if ends[k] - cur >= pn:
                    break
        if nl == 0:
            host += lens[i]
            i += 1
        else:
            linked += nl
            i += nl
    return linked, host


# ---- item 1: every symbol a hole of a hole, at the farthest distance -------------------------------------------------

def far_hole_chain(nseg=130, matches=3, dist=WINDOW):
    """32 768 stored bytes, then nseg flush-terminated segments of `matches` 258-byte matches at distance `dist` (fixed
    codes: length code 285, distance code 29 with 13 extra bits): every symbol of those segments is a hole, a segment is
    shorter than the distance, so each hole's byte lies some 42 segments back and is, from there on, a hole itself."""
    s = Stream()
    s.stored(noise(WINDOW, 1))
    for _ in range(nseg):
        s.fixed()
        for _ in range(matches):
            s.match(258, dist)
        s.end_block()
        s.stored()
    return s.result(s.finish(), far=dist, seg_len=258 * matches)


# ---- item 2: holes whose byte lies several tiny segments back ---------------------------------------------------------

def tiny_segments(rounds=24):
    """Segments of 0, 1, 2 and 3 output bytes (consecutive flush markers give empty ones) between a stored stretch and
    segments whose matches reach across them: consecutive holes of one match take their bytes from the long segment,
    the 1-, 2- and 3-byte segments and -- past two empty ones -- land in their own segment; the next segment copies
    those holes again."""
    s = Stream()
    s.stored(noise(300, 2))
    far = []  # (segment index, distance) of the matches that reach across the tiny segments
    for r in range(rounds):
        s.stored()
        for k in (1, 2, 3):
            s.fixed()
            for q in range(k):
                s.lit(65 + (r * 7 + k * 3 + q) % 26)
            s.end_block()
            s.stored()
        s.stored()
        s.stored()
        far.append((len(s.lens), 46))
        s.fixed()
        s.match(50, 46)  # 40 bytes in front of the tiny run, its 6 bytes, then 4 of the segment's own
        s.lit(97 + r % 26)
        s.end_block()
        s.stored()
        s.fixed()
        s.match(20, 25)  # holes of the holes just made
        s.match(3, 80 + r % 5)
        s.end_block()
        s.stored()
    return s.result(s.finish(), far=far)


# ---- item 3: the window in front of a piece, and the member's start ---------------------------------------------------

def window_edge(first, beyond=0):
    """Two segments that pieces of 64 KiB must take one at a time: `first` stored bytes, then a fixed block whose first
    match reaches min(first, 32 768) + beyond bytes back from the segment's first byte -- the oldest byte of the window
    the second piece is given, or (beyond = 1, first < 32 768) one byte in front of the member -- followed by matches
    onto the window's newest byte and its middle, and a stored stretch that carries the segment past the first piece's
    end.  (With first >= 32 768 one byte further would be distance 32 769, which DEFLATE cannot express.)"""
    s = Stream()
    s.stored(noise(first, 3))
    wlen = min(first, WINDOW)
    s.fixed()
    s.match(258, wlen + beyond)
    s.match(7, 258 + 1)            # the window's newest byte
    s.match(100, 265 + wlen // 2)  # its middle
    s.match(258, min(WINDOW, 365 + wlen))
    s.end_block()
    s.stored(noise(PIECE_FLOOR + 5000 - first if first < 40000 else 30000, 4))
    r = s.result(s.finish(), wlen=wlen)
    assert r["starts"][1] < PIECE_FLOOR < r["starts"][2]  # the second segment straddles the first piece's end
    return r


def reach_before_member(lead, pad=0):
    """A good member of 40 000 bytes, then a member whose first segments (`lead` stored bytes, then a match at distance
    lead + 100) reach 100 bytes in front of its own start, where the first member's bytes lie in the output; `pad`
    stored bytes follow (block mode takes members of 1 MiB and more)."""
    a = Stream()
    a.stored(noise(40000, 5))
    good = a.result(a.finish())
    s = Stream()
    if lead:
        s.stored(noise(lead, 6))
    s.fixed()
    s.match(258, lead + 100)
    s.end_block()
    s.stored()
    for k in range(0, pad, 65535):
        s.stored(noise(min(65535, pad - k), 7 + k, 32, 128))
    bad = s.result(s.finish())
    assert bad["data"] is None
    return dict(gz=good["gz"] + bad["gz"], data=None, raw=bad["raw"], good=good)


# ---- item 4: more false candidates than the scan keeps ---------------------------------------------------------------

def dense_false_candidates(n=1280 << 10):
    """gzip level 0's shape (stored blocks of 65 535 bytes: every block a segment) around a payload of 00 00 FF FF: an
    empty stored block at every fourth byte and, two bytes on, FF FF 00 00 -- a stored header of length 65 535 after a
    byte below 32 -- so about two candidates per four bytes."""
    s = Stream()
    payload = b"\x00\x00\xff\xff" * (n // 4)
    for k in range(0, n, 65535):
        s.stored(payload[k:k + 65535])
    return s.result(s.finish())


# ---- item 5: slot capacity ---------------------------------------------------------------------------------------------

def zlib_flushed(data, seg_lens, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15):
    """zlib's raw DEFLATE of data with a Z_SYNC_FLUSH after each of seg_lens bytes, closed by a final empty stored block."""
    assert sum(seg_lens) == len(data)
    c = zlib.compressobj(level, zlib.DEFLATED, -wbits, 9, strategy)
    raw, starts, at = b"", [0], 0
    for n in seg_lens:
        raw += c.compress(data[at:at + n]) + c.flush(zlib.Z_SYNC_FLUSH)
        starts.append(len(raw))
        at += n
    raw += FINAL_EMPTY_STORED
    return dict(gz=member(raw, data), data=data, raw=raw, starts=starts, lens=list(seg_lens) + [0])


SLOT_PATTERNS = {
    "exact": [SLOT_SYMS] * 5,
    "one_over": [SLOT_SYMS + 1] * 5,
    "alternating": [SLOT_SYMS, SLOT_SYMS + 1, 1000, SLOT_SYMS + 1, SLOT_SYMS + 1, SLOT_SYMS, 30000, SLOT_SYMS, SLOT_SYMS + 2, 5,
                    SLOT_SYMS - 1, 70000, 69000],
}


def slot_capacity(kind):
    lens = SLOT_PATTERNS[kind]
    return zlib_flushed(text(sum(lens), 8), lens)


def long_block(rle=False):
    """Block mode: 1.1 MiB that zlib stores (a member of kSplitMinBytes and more), then a run of 3 MiB that it packs
    into blocks far longer than a block slot."""
    data = noise(1100 << 10, 9) + (b"\x07" * (3 << 20) if rle else bytes(3 << 20))
    c = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_RLE if rle else zlib.Z_DEFAULT_STRATEGY)
    raw = c.compress(data) + c.flush()
    return dict(gz=member(raw, data), data=data, raw=raw)


# ---- item 6: pieces that end inside a segment, or exactly on its end --------------------------------------------------

def piece_cuts(kind):
    """Stored blocks against pieces of 64 KiB (payload bytes 32..127: no false candidates).  "level0": 65 535 bytes a
    block as gzip -0 writes them, 65 540 with the header, so no piece holds a whole segment; "on_piece_end": blocks of
    65 536 bytes with their header, each ending on its piece's last byte; "final_on_piece_end": the same with the final
    block's end on a piece's last byte."""
    s = Stream()
    if kind == "level0":
        for k in range(6):
            s.stored(noise(65535, 20 + k, 32, 128))
        raw = s.finish()
    elif kind == "on_piece_end":
        for k in range(5):
            s.stored(noise(PIECE_FLOOR - 5, 30 + k, 32, 128))
        raw = s.finish()
    else:
        for k in range(3):
            s.stored(noise(PIECE_FLOOR - 5, 40 + k, 32, 128))
        s.stored(noise(PIECE_FLOOR - 5, 43, 32, 128), final=True)
        raw = s.finish(marker=False)
        assert len(raw) == 4 * PIECE_FLOOR
    return s.result(raw)


# ---- item 7: what the corpora never give the decode kernel ------------------------------------------------------------

def single_distance(dist, nseg=3, matches=250):
    """Dynamic blocks whose distance code is a single one-bit code (the code of `dist`), each 32 literals and then
    `matches` 258-byte matches at distances in that code's range starting from `dist`."""
    sym, eb, _ = distance_symbol(dist)
    dists = [d for d in range(dist, DBASE[sym] + (1 << eb))][:2]
    lit_lens = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 6  # the fixed code's lengths, 286 symbols: complete
    lit_lens[284], lit_lens[285] = 7, 7                    # (286 and 287 are gone: two 7-bit codes make it complete again)
    dist_lens = [0] * sym + [1]
    s = Stream()
    for k in range(nseg):
        s.dynamic(lit_lens, dist_lens)
        for q in range(32):
            s.lit((k * 37 + q * 11) % 256)
        for q in range(matches):
            s.match(258, dists[q % len(dists)])
        s.end_block()
        s.stored()
    return s.result(s.finish(), dist_codes=1, dists=sorted(s.dists_used))


def long_codes(nseg=6, ops=6000, seed=12):
    """Dynamic blocks whose literal/length and distance codes both run to 15 bits (ladder()), all 256 literals, every
    length and distance in use; a segment per block, matches reaching in front of it included."""
    rng = np.random.default_rng(seed)
    s = Stream()
    s.stored(noise(40000, seed + 1))
    for k in range(nseg):
        s.dynamic(ladder(286, seed + 2 + k), ladder(30, seed + 50 + k))
        kinds = rng.integers(0, 4, size=ops)
        vals = rng.integers(0, 1 << 30, size=(ops, 2))
        for q in range(ops):
            if kinds[q] < 3:
                s.lit(int(vals[q, 0]) & 255)
            else:
                d = DBASE[int(vals[q, 1]) % 30]
                d += int(vals[q, 0]) % (1 << DEXT[distance_symbol(d)[0]])
                n = 258 if (int(vals[q, 1]) >> 20) % 16 == 0 else 3 + (int(vals[q, 0]) >> 8) % 32
                s.match(n, min(d, len(s.out), WINDOW))
        s.end_block()
        s.stored()
        assert s.lens[-1] <= SLOT_SYMS
    return s.result(s.finish(), lit_max=max(s.lit_lens_used), dist_max=max(s.dist_lens_used))


def decode_streams():
    """name -> stream, each cut by flush points into several segments that fit a slot."""
    t = text(200000, 13)
    mix = t[:60000] + noise(20000, 14) + bytes(20000) + t[60000:110000]
    return {
        "fixed": zlib_flushed(t, [25000] * 8, 6, zlib.Z_FIXED),
        "huffman_only": zlib_flushed(mix, [25000] * 6, 6, zlib.Z_HUFFMAN_ONLY),
        "wbits9": zlib_flushed(t, [40000] * 5, 6, zlib.Z_DEFAULT_STRATEGY, 9),
        "long_codes": long_codes(),
        "distance_1": single_distance(1),
        "distance_15_16": single_distance(15),
        "distance_17": single_distance(17),
    }


# ---- item 8: the block scan at tile, halo and piece edges -------------------------------------------------------------

def header_bits(kind):
    """(value, bits) of a dynamic block header, first bit in bit 0.  "min": the shortest the checker accepts, 91 bits --
    256 zero lengths in two repeats, a one-bit code for the end-of-block symbol, no distance code; "long": 2233 bits,
    every literal/length length at a seven-bit precode symbol, which needs nearly the whole halo; "stub": 29 bits that
    pass the cheap half of the test (a complete precode of four two-bit codes) and can never pass the walk."""
    w = BitWriter()
    if kind == "min":
        dynamic_header(w, 0, 257, 1, [(18, 127), (18, 107), 1, 0], {18: 1, 1: 2, 0: 2})
    elif kind == "long":
        dynamic_header(w, 0, 286, 30, [8] * 226 + [9] * 60 + [4] * 2 + [5] * 28, {18: 1, 17: 2, 16: 3, 0: 4, 4: 5, 5: 6, 8: 7, 9: 7})
    else:
        dynamic_header(w, 0, 257, 1, [], {16: 2, 17: 2, 18: 2, 0: 2})
    bits = len(w.out) * 8 + w.n
    return int.from_bytes(bytes(w.out), "little") | w.bits << (len(w.out) * 8), bits


def head_ok(buf, bit):
    """inflate_core.h inf_dynamic_head restated: BTYPE 2, HLIT and HDIST in range, a complete precode."""
    w = int.from_bytes(buf[bit >> 3:(bit >> 3) + 12], "little") >> (bit & 7)
    if (w >> 1) & 3 != 2 or (w >> 3) & 31 > 29 or (w >> 8) & 31 > 29:
        return False
    kraft = 0
    for i in range(((w >> 13) & 15) + 4):
        l = (w >> (17 + 3 * i)) & 7
        kraft += (128 >> l) if l else 0
    return kraft == 128


def scan_stream(plants, tail=None):
    """A valid gzip stream of stored blocks of zeros with block headers planted at exact bit offsets of its payload:
    plants = [(bit offset in the member's raw stream, header kind)].  zlib decodes it; the block scan tests every bit
    offset whether a block starts there or not.
    tail None: a member of 20 000 bytes that the first piece's chain decodes whole, then a member just under 1 MiB
    (decoded serially: it is never scanned), so the call scans exactly one piece: the first 1 MiB of the first member's
    stream, most of which is the second member's payload.
    tail R: one member, 16 stored blocks of 65 535 bytes and a final one sized so that the first piece (1 MiB) ends
    inside the 16th and the second and last piece -- from that block's start -- is R bytes long.
    -> gz, data, pieces: the (offset, length) in gz of each piece the scan sees, plants."""
    if tail is None:
        sizes_a, final_a = [20000], 0
        nb = SPLIT_MIN - 4000
        sizes_b = [65535] * ((nb - 23) // 65540)
        sizes_b.append(nb - 23 - 65540 * len(sizes_b))
    else:
        sizes_a, final_a, sizes_b = [65535] * 16, tail - 65540 - 5 - 8, None
        assert 0 <= final_a <= 65535
    buf = bytearray(GZ_HEADER)
    ranges = []  # payload ranges (gz offsets) of everything

    def blocks(sizes, final_len):
        first = len(ranges)
        for n in sizes:
            buf.extend(b"\x00" + struct.pack("<HH", n, n ^ 0xffff))
            ranges.append((len(buf), len(buf) + n))
            buf.extend(bytes(n))
        buf.extend(b"\x01" + struct.pack("<HH", final_len, final_len ^ 0xffff))
        ranges.append((len(buf), len(buf) + final_len))
        buf.extend(bytes(final_len))
        crc_at = len(buf)
        buf.extend(bytes(8))
        return first, len(ranges), crc_at

    members = [blocks(sizes_a, final_a)]
    if sizes_b:
        buf.extend(GZ_HEADER)
        members.append(blocks(sizes_b[:-1], sizes_b[-1]))
    for bit, kind in plants:
        v, nbits = header_bits(kind)
        lo, hi = 10 + (bit >> 3), 10 + ((bit + nbits + 7) >> 3)
        assert any(a <= lo and hi <= b for a, b in ranges), "a planted header must lie inside one stored payload"
        v <<= bit & 7
        old = int.from_bytes(buf[lo:hi], "little")
        buf[lo:hi] = (old | v).to_bytes(hi - lo, "little")
    data = b""
    for first, last, crc_at in members:
        d = b"".join(bytes(buf[a:b]) for a, b in ranges[first:last])
        buf[crc_at:crc_at + 8] = struct.pack("<II", zlib.crc32(d), len(d))
        data += d
    gz = bytes(buf)
    if tail is None:
        assert len(gz) - 10 >= SPLIT_MIN and len(gz) - members[1][2] < 8 + 1  # (the second member ends the stream)
        assert len(gz) - (members[0][2] + 8) - 10 < SPLIT_MIN
        pieces = [(10, SPLIT_MIN)]
    else:
        b0 = 10 + 15 * 65540
        assert len(gz) - b0 == tail
        pieces = [(10, SPLIT_MIN), (b0, tail)]
    return dict(gz=gz, data=data, pieces=pieces, plants=list(plants))


SCAN_EDGE_TILE = 40    # the tile edge the edge series crosses: byte 163 840 of the piece, inside a stored payload
SCAN_EDGE_RANGE = range(-16, 16)
SCAN_HALO_RANGE = range(-2, 2)
SCAN_TAILS = (81920, 81919, 81921, 81923)  # 4096 k, 4096 k - 1, + 1, + 3


def scan_edge(delta):
    """A shortest header starting `delta` bits from a tile edge: the last 16 bits of a tile, the first 16 of the next."""
    return scan_stream([(8 * SCAN_TILE * SCAN_EDGE_TILE + delta, "min")])


def scan_halo(delta):
    """The long header starting `delta` bits from a tile edge: on a tile's last bit (delta -1) it ends 2232 bits into
    the halo."""
    return scan_stream([(8 * SCAN_TILE * SCAN_EDGE_TILE + delta, "long")])


def scan_piece_end(delta, kind="long"):
    """A header that ends `delta` bits from the piece's last bit: 0 ends exactly on it, 1 is one bit too long (refused:
    the header must lie inside the piece), -1 and -9 fit."""
    return scan_stream([(8 * SPLIT_MIN + delta - header_bits(kind)[1], kind)])


def scan_dense(count=600, start_tile=60):
    """Back-to-back stretch from a tile's first bit: per shortest header two stubs that pass only the cheap half, so a
    wave queues about 165 survivors a quarter tile and flushes 64 of them twice with a remainder."""
    at, plants = 8 * SCAN_TILE * start_tile, []
    for _ in range(count):
        plants += [(at, "min"), (at + 91, "stub"), (at + 120, "stub")]
        at += 149
    return scan_stream(plants)


def scan_overflow(count=21000, start_tile=60):
    """More accepted headers (back to back, 91 bits each) than the scan's candidate list holds: P / 64 + 4096 = 20 480
    for a piece of 1 MiB."""
    at0 = 8 * SCAN_TILE * start_tile
    plants, at = [], at0
    while len(plants) < count:
        lo = 10 + (at >> 3)
        # (skip the stored blocks' own headers: a planted header lies inside one payload)
        if (lo - 10 - 20018 - 10) % 65540 > 65540 - 24 or (lo - 10 - 20018 - 10) % 65540 < 8:
            at += 8 * 40
            continue
        plants.append((at, "min"))
        at += 91
    return scan_stream(plants)


def scan_tail(length):
    """Two pieces, the second `length` bytes long (the byte-wise tail of the last tile's load), with shortest headers on
    the last bits in front of the member's trailer and at the last full tile's edge."""
    b0 = 15 * 65540
    end = 8 * (b0 + length - 8)  # the first bit of the trailer
    edge = 8 * (b0 + 19 * SCAN_TILE)  # (inside the final block's payload for every length in SCAN_TAILS)
    return scan_stream([(end - 91, "min"), (end - 91 - 300, "min"), (edge - 5, "min"), (edge - 2300, "long")], tail=length)
