"""Builders of .xz files for the xz tests (test_xz_host.py on the CPU, test_gpu_unxz.py / test_gpu_xz_edges.py on the
GPU): no asserts about the library here, only about the files themselves.

xz_file() takes raw LZMA2 from liblzma (lzma.compress(format=FORMAT_RAW)) and wraps it in its own Block headers, Index,
footer and Stream Padding, so that the tests decide how many Blocks and Streams a file has, which Check it carries and
whether the Block headers state their sizes.  Every file of good_cases() is run through liblzma before it is returned,
every file of bad_cases() is one liblzma refuses, every file of unsupported_cases() is one it accepts.

The reference is liblzma through Python's lzma module.  ref_decompress() drives it the way the xz tool does (one
LZMADecompressor(FORMAT_XZ) per Stream, Stream Padding of four zero bytes at a time between and after Streams, anything
else an error) because lzma.decompress()'s own loop, not liblzma, gives up on the first byte of Stream Padding and
silently drops trailing bytes that do not begin a Stream.  Where a file has neither, lzma.decompress() itself is asked
too; the bad cases whose verdict is the loop's and not liblzma's are marked strict_only."""
import functools
import hashlib
import lzma
import random
import struct
import zlib

CHECK_NONE, CHECK_CRC32, CHECK_CRC64, CHECK_SHA256 = 0, 1, 4, 10
MAGIC = b"\xfd7zXZ\x00"


def crc64(data, crc=0):
    """CRC-64/XZ, bit by bit."""
    c = crc ^ 0xFFFFFFFFFFFFFFFF
    for b in data:
        c ^= b
        for _ in range(8):
            c = (c >> 1) ^ (0xC96C5795D7870F42 if c & 1 else 0)
    return c ^ 0xFFFFFFFFFFFFFFFF


@functools.lru_cache(maxsize=None)
def _crc64_table():
    t = []
    for b in range(256):
        c = b
        for _ in range(8):
            c = (c >> 1) ^ (0xC96C5795D7870F42 if c & 1 else 0)
        t.append(c)
    return t


def crc64_fast(data):
    """The same by a byte table built from the bitwise definition (for the larger expected values)."""
    t = _crc64_table()
    c = 0xFFFFFFFFFFFFFFFF
    for b in data:
        c = (c >> 8) ^ t[(c ^ b) & 0xFF]
    return c ^ 0xFFFFFFFFFFFFFFFF


assert crc64(b"123456789") == 0x995DC9BBDF1939FA == crc64_fast(b"123456789")
assert struct.pack("<Q", crc64(b"abc")) in lzma.compress(b"abc", check=lzma.CHECK_CRC64)[-36:-20]  # the Check field liblzma wrote


def ref_decompress(z):
    """liblzma's verdict on a whole file, Streams and Stream Padding read as the xz tool reads them."""
    out = []
    data = z
    while True:
        d = lzma.LZMADecompressor(lzma.FORMAT_XZ)
        out.append(d.decompress(data))
        if not d.eof:
            raise lzma.LZMAError("input ends inside a Stream")
        data = d.unused_data
        while len(data) >= 4 and data[:4] == b"\0\0\0\0":
            data = data[4:]
        if not data:
            return b"".join(out)


def refuses(fn, z):
    try:
        fn(z)
    except (lzma.LZMAError, EOFError):
        return True
    return False


def vli(v):
    out = bytearray()
    while v >= 0x80:
        out.append(v & 0x7F | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def dict_byte(dict_size):
    for b in range(41):
        if (0xFFFFFFFF if b == 40 else (2 | (b & 1)) << (b // 2 + 11)) >= dict_size:
            return b
    raise ValueError(dict_size)


def raw_lzma2(data, dict_size=1 << 20, **opts):
    """(raw LZMA2 with its end byte, the data, the dictionary size) -- a Block for xz_file."""
    f = dict(id=lzma.FILTER_LZMA2, dict_size=max(dict_size, 4096))
    f.update(opts)
    return lzma.compress(data, format=lzma.FORMAT_RAW, filters=[f]), data, max(dict_size, 4096)


def check_field(check, data):
    if check == CHECK_NONE:
        return b""
    if check == CHECK_CRC32:
        return struct.pack("<I", zlib.crc32(data))
    if check == CHECK_CRC64:
        return struct.pack("<Q", crc64_fast(data))
    if check == CHECK_SHA256:
        return hashlib.sha256(data).digest()
    return bytes({2: 4, 3: 4, 5: 8, 6: 8}.get(check, 16))


def block_header(dict_size, csize=None, usize=None, filters=None):
    flags = (0x40 if csize is not None else 0) | (0x80 if usize is not None else 0)
    body = b""
    if csize is not None:
        body += vli(csize)
    if usize is not None:
        body += vli(usize)
    body += b"\x21\x01" + bytes([dict_byte(dict_size)])
    n = 2 + len(body) + 4
    n = (n + 3) & ~3
    h = bytes([n // 4 - 1, flags]) + body
    h += bytes(n - 4 - len(h))
    return h + struct.pack("<I", zlib.crc32(h))


def index_field(records):
    ix = b"\x00" + vli(len(records)) + b"".join(vli(u) + vli(n) for u, n in records)
    ix += bytes(-len(ix) % 4)
    return ix + struct.pack("<I", zlib.crc32(ix))


class Stream:
    """One Stream's bytes and where its parts lie (offsets into .data)."""

    def __init__(self, blocks, check=CHECK_CRC64, sizes_in_header=False, records=None, count=None):
        flags = bytes([0, check])
        d = bytearray(MAGIC + flags + struct.pack("<I", zlib.crc32(flags)))
        self.parts = []
        recs = []
        for raw, data, dict_size in blocks:
            h = block_header(dict_size, len(raw) if sizes_in_header else None, len(data) if sizes_in_header else None)
            ck = check_field(check, data)
            p = dict(hdr=len(d), data=len(d) + len(h), pad=len(d) + len(h) + len(raw))
            unpadded = len(h) + len(raw) + len(ck)
            d += h + raw + bytes(-(len(h) + len(raw)) % 4)
            p["check"] = len(d)
            d += ck
            p["end"] = len(d)
            self.parts.append(p)
            recs.append((unpadded, len(data)))
        if records is not None:
            recs = records(recs)
        ix = index_field(recs)
        if count is not None:  # a record count that disagrees with the records, under a valid CRC
            body = b"\x00" + vli(count) + b"".join(vli(u) + vli(n) for u, n in recs)
            body += bytes(-len(body) % 4)
            ix = body + struct.pack("<I", zlib.crc32(body))
        self.index = len(d)
        d += ix
        self.footer = len(d)
        tail = struct.pack("<I", len(ix) // 4 - 1) + flags
        d += struct.pack("<I", zlib.crc32(tail)) + tail + b"YZ"
        self.data = bytes(d)
        self.plain = b"".join(b[1] for b in blocks)


def xz_file(blocks, check=CHECK_CRC64, sizes_in_header=False, padding=0):
    """One Stream of the given Blocks (raw_lzma2 triples) followed by `padding` bytes of Stream Padding."""
    return Stream(blocks, check, sizes_in_header).data + bytes(padding)


# ---- data ------------------------------------------------------------------------------------------------------------

WORDS = ("snap click package install verify archive member digest block stream header footer index record kernel lane wave "
         "buffer offset length distance literal match repeat dictionary reset state chunk control properties").split()


def text(n, seed=1):
    r = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        k = r.randrange(100)
        if k < 70:
            out += r.choice(WORDS).encode() + b" "
        elif k < 80:
            out += b"%s=%d\n" % (r.choice(WORDS).encode(), r.randrange(1000))
        elif k < 90:
            out += b"key_%02d: value_%02d\n" % (r.randrange(8), r.randrange(4))
        else:
            out += bytes(r.randrange(256) for _ in range(r.randrange(1, 6)))
    return bytes(out[:n])


def rnd(n, seed=2):
    return random.Random(seed).randbytes(n)


def periodic(dist, length, seed=3, tail=b""):
    """`dist` distinct-ish bytes, then `length` more that continue the period: a match of that distance and length whose
    distance equals the bytes produced so far."""
    r = random.Random(seed * 1000 + dist)
    base = bytes(r.sample(range(256), dist)) if dist <= 256 else r.randbytes(dist)
    return base + bytes(base[i % dist] for i in range(length)) + tail


def sprinkled(dist, length, seed=4, times=40):
    """Random bytes (literals are dear there) with `times` copies of `length` bytes from `dist` back sprinkled in, after one
    long copy from the same distance: what makes the encoder spend a (rep) match on two bytes."""
    r = random.Random(seed * 1000 + dist * 10 + length)
    out = bytearray(r.randbytes(400))
    for _ in range(30):  # a long copy first: the distance is then a rep distance, which two bytes can afford
        out.append(out[-dist])
    out += r.randbytes(3)
    for _ in range(times):
        for _ in range(length):
            out.append(out[-dist])
        while True:  # a byte that ends the match
            b = r.randrange(256)
            if b != out[-dist]:
                break
        out.append(b)
        out += r.randbytes(5)
    return bytes(out)


# ---- chunk surgery on raw LZMA2 ----------------------------------------------------------------------------------------

def join_raw(a, b, second_control=None):
    """Two independently compressed raw LZMA2 streams as the chunks of ONE Block: a's end byte dropped, b's first chunk
    keeping its E0 (dictionary reset, new properties), or rewritten to C0 (state reset + properties) or A0 (state reset;
    the properties byte removed: the streams must share them).  For C0 / A0 the positions go on counting, so a's length
    must be a multiple of 16 and end in a zero byte (the literal coder's context at b's first byte is then what b's encoder
    saw)."""
    ra, da, dict_a = a
    rb, db, dict_b = b
    assert ra[-1] == 0 and rb[0] >= 0xE0
    if second_control is not None:
        assert len(da) % 16 == 0 and da[-1] == 0
        rb = bytes([second_control | (rb[0] & 0x1F)]) + rb[1:]
        if second_control == 0xA0:
            rb = rb[:5] + rb[6:]
    return ra[:-1] + rb, da + db, max(dict_a, dict_b)


# ---- a range encoder of its own, for the chunk liblzma's encoder never writes ----------------------------------------------

class _RangeEncoder:
    """The LZMA range encoder, enough of it to write one literal and a run of matches (lc=3 lp=0 pb=2)."""

    def __init__(self):
        self.low, self.range, self.cache, self.cache_size, self.out = 0, 0xFFFFFFFF, 0, 1, bytearray()
        self.probs = [1024] * (1846 + (0x300 << 3))

    def _shift_low(self):
        if self.low < 0xFF000000 or self.low >= 1 << 32:
            carry = self.low >> 32
            while self.cache_size:
                self.out.append((self.cache + carry) & 0xFF)
                self.cache = 0xFF
                self.cache_size -= 1
            self.cache = (self.low >> 24) & 0xFF
        self.cache_size += 1
        self.low = (self.low & 0x00FFFFFF) << 8

    def bit(self, index, b):
        p = self.probs[index]
        bound = (self.range >> 11) * p
        if b == 0:
            self.range = bound
            self.probs[index] = p + ((2048 - p) >> 5)
        else:
            self.low += bound
            self.range -= bound
            self.probs[index] = p - (p >> 5)
        while self.range < 1 << 24:
            self.range = (self.range << 8) & 0xFFFFFFFF
            self._shift_low()

    def tree(self, base, nbits, value):
        m = 1
        for i in range(nbits - 1, -1, -1):
            b = value >> i & 1
            self.bit(base + m, b)
            m = m << 1 | b

    def finish(self):
        for _ in range(5):
            self._shift_low()
        return bytes(self.out)


def run_chunk(byte, n):
    """One LZMA2 chunk (dictionary reset, new properties) of `n` bytes `byte`, n from 3 to 2 MiB: a literal, a match of
    distance 1, then rep0 matches of 273 bytes -- with its end byte, a Block for xz_file.  The probability offsets are
    those of the LZMA description (IsMatch 0, IsRep 192, IsRepG0 204, IsRep0Long 240, PosSlot 432, the length coders at
    818 and 1332, the literals at 1846)."""
    assert 3 <= n <= 1 << 21
    rc = _RangeEncoder()
    rc.bit(0, 0)                                  # IsMatch[state 0][pos_state 0]: a literal, context 0
    rc.tree(1846, 8, byte)
    pos, state, first = 1, 0, True
    while pos < n:
        ln = min(273, n - pos)
        if n - pos - ln == 1:                     # (one byte cannot be a match: leave two for the last one)
            ln -= 1
        ps = pos & 3
        rc.bit(0 + (state << 4) + ps, 1)          # IsMatch
        if first:
            rc.bit(192 + state, 0)                # IsRep: a new match
            lenbase = 818
        else:
            rc.bit(192 + state, 1)                # a rep ...
            rc.bit(204 + state, 0)                # ... of rep0 ...
            rc.bit(240 + (state << 4) + ps, 1)    # ... longer than one byte
            lenbase = 1332
        if ln < 10:
            rc.bit(lenbase, 0)
            rc.tree(lenbase + 2 + (ps << 3), 3, ln - 2)
        elif ln < 18:
            rc.bit(lenbase, 1)
            rc.bit(lenbase + 1, 0)
            rc.tree(lenbase + 130 + (ps << 3), 3, ln - 10)
        else:
            rc.bit(lenbase, 1)
            rc.bit(lenbase + 1, 1)
            rc.tree(lenbase + 258, 8, ln - 18)
        if first:
            rc.tree(432 + (min(ln - 2, 3) << 6), 6, 0)  # distance slot 0: distance 1
            state = 7 if state < 7 else 10
        else:
            state = 8 if state < 7 else 11
        first = False
        pos += ln
    body = rc.finish()
    assert len(body) <= 1 << 16
    head = bytes([0xE0 | (n - 1) >> 16, (n - 1) >> 8 & 0xFF, (n - 1) & 0xFF, (len(body) - 1) >> 8, (len(body) - 1) & 0xFF, 0x5D])
    return head + body + b"\x00", bytes([byte]) * n, 4096


# ---- the cases -----------------------------------------------------------------------------------------------------------

COPY_DISTS = (1, 63, 64, 65)
COPY_LENS = (2, 64, 65, 273)
GREEDY = dict(mode=lzma.MODE_NORMAL, mf=lzma.MF_BT4, nice_len=273, depth=0)


def _good(name, z, plain, padded=False):
    assert ref_decompress(z) == plain, name
    if not padded:
        assert lzma.decompress(z) == plain, name
    return name, z, plain


@functools.lru_cache(maxsize=None)
def edge_cases():
    """(name, file, plain bytes): the shapes at which the decoder and the kernel's wave copy can go wrong, each as small
    as it can be.  test_xz_host.py asserts from the harness's histogram that each shape occurred."""
    out = []
    for d in COPY_DISTS:
        for ln in COPY_LENS:
            data = sprinkled(d, ln) if ln == 2 else periodic(d, ln, tail=rnd(7, d * 300 + ln))
            out.append(_good("copy_d%d_l%d" % (d, ln), xz_file([raw_lzma2(data, **GREEDY)]), data))
    data = rnd(4096, 5) + rnd(4096, 5)[:80] + b"end"
    out.append(_good("dist_is_dict_size", xz_file([raw_lzma2(data, dict_size=4096, **GREEDY)]), data))
    t = text(60000, 6)
    out.append(_good("reps", xz_file([raw_lzma2(t)]), t))
    for name, o in (("lc4_lp0", dict(lc=4, lp=0)), ("lc0_lp4", dict(lc=0, lp=4)), ("pb0", dict(pb=0)), ("pb4", dict(pb=4))):
        out.append(_good(name, xz_file([raw_lzma2(t[:20000], **o)]), t[:20000]))
    out.append(_good("one_byte", xz_file([raw_lzma2(b"x")]), b"x"))
    z2m = bytes(range(256)) * 8192 + text(3000, 7)  # the first chunk is as long as liblzma's encoder makes one: just under 2 MiB
    out.append(_good("chunk_near_2mib", xz_file([raw_lzma2(z2m)]), z2m))
    blk = run_chunk(0x5A, 1 << 21)  # the 21-bit size field at all ones: liblzma's encoder stops short of it, this one does not
    out.append(_good("chunk_2mib", xz_file([blk]), blk[1]))
    r = rnd(150000, 8)
    out.append(_good("uncompressed_chunks", xz_file([raw_lzma2(r)]), r))
    big = text(2621440, 9)  # 2.5 MiB in one Block: chunks 80-9F continue the probabilities
    out.append(_good("chunks_continue", xz_file([raw_lzma2(big)]), big))
    a = text(4095, 10) + b"\0"
    b = text(3000, 11)
    out.append(_good("e0_mid_block", xz_file([join_raw(raw_lzma2(a, lc=3, pb=2), raw_lzma2(b, lc=1, lp=2, pb=1))]), a + b))
    out.append(_good("c0_mid_block", xz_file([join_raw(raw_lzma2(a, lc=3, pb=2), raw_lzma2(b, lc=1, lp=2, pb=1), 0xC0)]), a + b))
    out.append(_good("a0_mid_block", xz_file([join_raw(raw_lzma2(a), raw_lzma2(b), 0xA0)]), a + b))
    for k in range(4):  # a Block's compressed length 0..3 mod 4: every padding
        blocks, n = [], 100
        while len(blocks) < 4:
            blk = raw_lzma2(text(n, 12 + k))
            n += 1
            if (len(blk[0]) + 12) % 4 == k:
                blocks.append(blk)
        out.append(_good("padding_%d" % k, xz_file(blocks), b"".join(x[1] for x in blocks)))
    t300 = text(300 * 4096, 13)
    out.append(_good("blocks_300", xz_file([raw_lzma2(t300[i:i + 4096]) for i in range(0, len(t300), 4096)]), t300))
    return out


@functools.lru_cache(maxsize=None)
def container_cases():
    """(name, file, plain bytes): every Check, sizes in the Block headers, Streams one after another with padding, a Stream
    without Blocks, and what lzma.compress writes by itself."""
    out = []
    t = text(50000, 20)
    blocks = [raw_lzma2(t[i:i + 12500]) for i in range(0, 50000, 12500)]
    for ck in (CHECK_NONE, CHECK_CRC32, CHECK_CRC64, CHECK_SHA256):
        out.append(_good("check_%d" % ck, xz_file(blocks, ck, sizes_in_header=ck != CHECK_CRC32), t))
    out.append(_good("empty_stream", xz_file([]), b""))
    out.append(_good("empty_block", xz_file([raw_lzma2(b"")]), b""))
    z = xz_file(blocks[:2], CHECK_CRC32, padding=8) + xz_file([], padding=4) + xz_file(blocks[2:], CHECK_SHA256) + bytes(12)
    out.append(_good("streams_padding", z, t, padded=True))
    out.append(_good("streams_no_padding", xz_file(blocks[:1]) + xz_file(blocks[1:], CHECK_NONE), t))
    for preset in (0, 6, 9 | lzma.PRESET_EXTREME):
        out.append(_good("liblzma_preset_%d" % (preset & 15), lzma.compress(t, preset=preset), t))
    return out


def good_cases():
    return edge_cases() + container_cases()


def _flip(z, at, bit=0x10):
    b = bytearray(z)
    b[at] ^= bit
    return bytes(b)


@functools.lru_cache(maxsize=None)
def bad_cases():
    """(name, file, strict_only): files liblzma refuses.  strict_only: refused by ref_decompress() (liblzma's concatenated
    reading) while lzma.decompress()'s loop drops the trailing bytes without a word."""
    t = text(30000, 30)
    blocks = [raw_lzma2(t[:15000]), raw_lzma2(t[15000:])]
    s = Stream(blocks, CHECK_CRC64, sizes_in_header=True)
    z, p0, p1 = s.data, s.parts[0], s.parts[1]
    out = [
        ("flip_stream_header", _flip(z, 7), False),
        ("flip_block_header", _flip(z, p0["hdr"] + 2), False),
        ("flip_block_header_crc", _flip(z, p0["data"] - 1), False),
        ("flip_payload", _flip(z, p0["data"] + 100), False),
        ("flip_payload_last_block", _flip(z, p1["data"] + 4000), False),
        ("flip_check", _flip(z, p1["check"] + 3), False),
        ("flip_index", _flip(z, s.index + 2), False),
        ("flip_index_crc", _flip(z, s.footer - 1), False),
        ("flip_footer", _flip(z, s.footer + 9), False),
        ("flip_footer_magic", _flip(z, len(z) - 1), False),
        ("flip_backward_size", _flip(z, s.footer + 4, 0x01), False),
    ]
    for k in range(4):  # a Block whose padding is 1..3 bytes, one of them set
        blk = next(b for n in range(100, 140) for b in [raw_lzma2(text(n, 31))] if (len(b[0]) + 12) % 4 == k)
        sp = Stream([blk, blk], CHECK_CRC32)
        if k:
            out.append(("flip_block_padding_%d" % (4 - k), _flip(sp.data, sp.parts[0]["pad"]), False))
    cuts = [0, 6, 12, p0["data"], p0["data"] + 50, p0["pad"], p0["check"], p0["end"], p1["data"] + 1000, s.index, s.index + 3, s.footer,
            s.footer + 4, len(z) - 2, len(z) - 1]
    out += [("cut_%d" % c, z[:c], False) for c in cuts]
    out += [
        ("junk_cut_header", z + MAGIC + b"ju", False),
        ("junk", z + b"junk", True),
        ("junk_after_padding", z + bytes(4) + b"junkjunk", True),
        ("second_stream_corrupt", z + _flip(z, 40), True),
        ("padding_1", z + bytes(1), False),
        ("padding_2", z + bytes(2), False),
        ("padding_3", z + bytes(3), False),
        ("padding_first", bytes(4) + z, False),
        ("index_disagrees_usize", Stream(blocks, records=lambda r: [(r[0][0], r[0][1] + 1), r[1]]).data, False),
        ("index_disagrees_unpadded", Stream(blocks, records=lambda r: [(r[0][0] + 1, r[0][1]), r[1]]).data, False),
        ("index_swapped", Stream(blocks, records=lambda r: r[::-1]).data, False),
        ("count_plus_one", Stream(blocks, count=3).data, False),
        ("count_minus_one", Stream(blocks, count=1).data, False),
        ("index_claims_2_60", Stream(blocks, records=lambda r: [r[0], (r[1][0], 1 << 60)]).data, False),
    ]
    raw, data, ds = blocks[0]
    out += [
        ("first_chunk_no_dict_reset", xz_file([(bytes([0xC0 | raw[0] & 0x1F]) + raw[1:], data, ds)]), False),
        ("first_chunk_uncompressed_no_reset", xz_file([(b"\x02\x00\x02abc\x00", b"abc", 4096)]), False),
        ("control_03", xz_file([(raw[:-1] + b"\x03", data, ds)]), False),
        ("control_03_first", xz_file([(b"\x03\x00\x02abc\x00", b"abc", 4096)]), False),
        ("no_end_byte", xz_file([(raw[:-1], data, ds)]), False),
        ("header_usize_wrong", Stream([(raw, data + b"x", ds)], CHECK_NONE, sizes_in_header=True).data, False),
        ("chunk_csize_minus_one", xz_file([(raw[:3] + struct.pack(">H", struct.unpack(">H", raw[3:5])[0] - 1) + raw[5:], data, ds)]), False),
        ("chunk_usize_minus_one", xz_file([(raw[:1] + struct.pack(">H", struct.unpack(">H", raw[1:3])[0] - 1) + raw[3:], data[:-1], ds)], CHECK_NONE), False),
        ("props_lc_lp_5", xz_file([(raw[:5] + bytes([4 + 9 * 1 + 45 * 2]) + raw[6:], data, ds)]), False),
    ]
    # a distance beyond what was produced: the chunks in front of an LZMA chunk that reaches back into them are dropped
    # (lc = lp = pb = 0: nothing of the decode depends on the position, so the first far match is what fails)
    pre = rnd(70000, 32)
    q = pre[:3000] + text(500, 33) + pre[5000:6000]
    raw2 = raw_lzma2(pre + q, lc=0, lp=0, pb=0)[0]
    at, first_lzma = 0, None
    while raw2[at] != 0:
        if raw2[at] >= 0x80:
            first_lzma = at
            break
        at += 3 + struct.unpack(">H", raw2[at + 1:at + 3])[0] + 1
    assert first_lzma and raw2[first_lzma] >= 0xC0
    far = bytes([0xE0 | raw2[first_lzma] & 0x1F]) + raw2[first_lzma + 1:]
    out.append(("distance_beyond_produced", xz_file([(far, q, 1 << 20)], CHECK_NONE), False))
    for name, bad, strict_only in out:
        assert refuses(ref_decompress, bad), name
        assert strict_only or refuses(lzma.decompress, bad), name
    return out


@functools.lru_cache(maxsize=None)
def unsupported_cases():
    """(name, file): well-formed files liblzma reads and this library hands back (SNAPHASH_EINVAL)."""
    t = text(20000, 40)
    x86 = lzma.compress(t, format=lzma.FORMAT_XZ, filters=[dict(id=lzma.FILTER_X86), dict(id=lzma.FILTER_LZMA2)])
    delta = lzma.compress(t, format=lzma.FORMAT_XZ, filters=[dict(id=lzma.FILTER_DELTA, dist=4), dict(id=lzma.FILTER_LZMA2)])
    check2 = xz_file([raw_lzma2(t)], check=2)
    out = [("x86_bcj", x86), ("delta", delta), ("check_id_2", check2)]
    for name, z in out:
        assert lzma.decompress(z) == t, name
    return out
