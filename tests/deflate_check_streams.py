"""Streams for the build side's self-check (snappy_amd/csrc/deflate_check_core.h), shared by tests/test_snapbuild_host.py
(the host walker) and tests/test_gpu_deflate_check_edges.py (deflate_check_kernel, which must answer the same bit for bit).

A case is (name, data, z, z_off, last_is_final, good): the staged stream, the compressed bytes, the nchunks + 1 offsets that
cut them into one stretch per 64 KiB chunk of data, whether the last chunk ends with the final block, and whether the case
is UNDAMAGED (every chunk must then be accepted).  zlib is the reference: zlib_accepts() decodes one chunk's stretch the
way the issue of the safety property is stated -- raw DEFLATE with the 32 KiB in front of the chunk as the dictionary, a
final empty stored block appended unless the stretch carries its own -- and says whether exactly the chunk came out and
the stream ended there."""
import random
import zlib

CHUNK = 65536
SIZES = (0, 1, 65535, 65536, 65537, 3 * 65536 + 1)
LEVELS = (0, 1, 9)
OK, LITERAL, MATCH, DISTANCE, BAD, LONG, SHORT, END, TABLE = range(9)
FINAL_EMPTY_STORED = b"\x01\x00\x00\xff\xff"

_WORDS = [w.encode() for w in ("snap click package hashes yaml sha512 archive control data member deflate chunk stored "
                               "dynamic fixed huffman literal match distance length window flush boundary").split()]


def payload(n, seed=7):
    """text with long-range repeats, binary runs and noise: dynamic blocks with matches that reach across chunk starts"""
    rnd = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        k = rnd.random()
        if k < 0.6:
            out += b" ".join(rnd.choice(_WORDS) for _ in range(rnd.randrange(3, 40))) + b"\n"
        elif k < 0.75 and len(out) > 40000:
            at = rnd.randrange(0, len(out) - 300)
            out += out[at:at + rnd.randrange(20, 300)]
        elif k < 0.9:
            out += bytes([rnd.randrange(256)]) * rnd.randrange(1, 70)
        else:
            out += bytes(rnd.randrange(256) for _ in range(rnd.randrange(1, 200)))
    return bytes(out[:n])


def nchunks_of(n):
    return max(1, (n + CHUNK - 1) // CHUNK)


def zlib_stream(data, level, final):
    """-> (z, z_off): raw DEFLATE of data, Z_SYNC_FLUSH after every 64 KiB (Z_FINISH after the last when final)"""
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    z, off = bytearray(), [0]
    nch = nchunks_of(len(data))
    for c in range(nch):
        z += co.compress(data[c * CHUNK:(c + 1) * CHUNK])
        z += co.flush(zlib.Z_FINISH if final and c == nch - 1 else zlib.Z_SYNC_FLUSH)
        off.append(len(z))
    return bytes(z), off


class Bits:
    """an LSB-first bit writer (RFC 1951 sec. 3.1.1); Huffman codes go in MSB first"""

    def __init__(self):
        self.bits = []

    def put(self, v, n):
        self.bits += [(v >> i) & 1 for i in range(n)]

    def code(self, v, n):
        self.bits += [(v >> (n - 1 - i)) & 1 for i in range(n)]

    def fixed_lit(self, s):
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def fixed_match3(self, dist_code, extra, extra_bits):
        self.fixed_lit(257)  # length 3, no extra bits
        self.code(dist_code, 5)
        self.put(extra, extra_bits)

    def align(self):
        while len(self.bits) % 8:
            self.bits.append(0)

    def bytes(self):
        self.align()
        return bytes(sum(b << i for i, b in enumerate(self.bits[k:k + 8])) for k in range(0, len(self.bits), 8))


def stored(data, final=False):
    assert len(data) < 65536
    return bytes([1 if final else 0]) + len(data).to_bytes(2, "little") + (len(data) ^ 0xffff).to_bytes(2, "little") + data


def fixed_block(tokens, sync=True):
    """tokens: ints (literals) and ("m3", dist_code, extra, extra_bits); BFINAL = 0, then the empty stored block"""
    b = Bits()
    b.put(0, 1)
    b.put(1, 2)
    for t in tokens:
        if isinstance(t, int):
            b.fixed_lit(t)
        else:
            b.fixed_match3(*t[1:])
    b.fixed_lit(256)
    if sync:
        b.put(0, 3)
        b.align()
        return b.bytes() + b"\x00\x00\xff\xff"
    return b.bytes()


DIST_32768 = ("m3", 29, 8191, 13)  # code 29: 24577 + 13 extra bits, all ones: the farthest distance RFC 1951 can say


def hand_built():
    """(name, data, z, z_off, final, good, want): want = the verdicts these must get, chunk by chunk (None: only the safety
    property is asked)"""
    out = []
    # the first match of chunk 1 reaches exactly 32 768 bytes back, into chunk 0
    d0 = payload(CHUNK, 11)
    d1 = d0[32768:32771] + b"xyz"
    z0, _ = zlib_stream(d0, 1, False)
    z1 = fixed_block([DIST_32768] + list(b"xyz"))
    out.append(("match_32768_into_previous_chunk", d0 + d1, z0 + z1, [0, len(z0), len(z0) + len(z1)], False, True, [(OK, CHUNK), (OK, 6)]))
    # the same distance with 32 768 / 32 767 bytes of the buffer in front of the match: chunk 0, behind a stored block
    for front, status in ((32768, OK), (32767, DISTANCE)):
        lits = payload(front, 12)
        data = lits + lits[:3] + b"!"
        z = stored(lits) + fixed_block([DIST_32768, ord("!")])
        good = status == OK
        out.append(("match_32768_with_%d_in_front" % front, data, z, [0, len(z)], False, good,
                    [(OK, front + 4) if good else (DISTANCE, front)]))
    # a match that reaches one byte in front of the buffer, and the one that just does not
    for dcode, status in ((2, OK), (3, DISTANCE)):  # distances 3 and 4 with 3 bytes in front
        z = fixed_block(list(b"abc") + [("m3", dcode, 0, 0), ord("X")])
        out.append(("match_dist_%d_with_3_in_front" % (dcode + 1), b"abcabcX", z, [0, len(z)], False, status == OK,
                    [(OK, 7) if status == OK else (DISTANCE, 3)]))
    # staged bytes changed under a fixed block: offset 0, the byte after the match, the last; and inside the match
    z = fixed_block(list(b"abc") + [("m3", 2, 0, 0), ord("X"), ord("Y")])
    for name, at, want in (("first", 0, (LITERAL, 0)), ("inside_match", 4, (MATCH, 4)), ("after_match", 6, (LITERAL, 6)), ("last", 7, (LITERAL, 7))):
        data = bytearray(b"abcabcXY")
        data[at] ^= 0x20
        out.append(("staged_byte_%s" % name, bytes(data), z, [0, len(z)], False, False, [want]))
    # fixed-Huffman distance codes 30 and 31 complete the code and are refused
    z = fixed_block(list(b"abc") + [("m3", 30, 0, 0)])
    out.append(("distance_code_30", b"abcabc", z, [0, len(z)], False, False, [(BAD, 3)]))
    # a block that ends on the stretch's last byte without the empty stored block: only accepted when it ends ON the boundary
    z = fixed_block(list(b"ab"), sync=False)
    out.append(("no_sync_block", b"ab", z, [0, len(z)], False, False, None))
    # BFINAL inside a chunk that is not the last of its member
    z = stored(b"hello", final=True)
    out.append(("bfinal_in_a_middle_chunk", b"hello", z, [0, len(z)], False, False, [(BAD, 0)]))
    out.append(("bfinal_in_the_last_chunk", b"hello", z, [0, len(z)], True, True, [(OK, 5)]))
    # more and fewer bytes than the chunk has
    z = stored(b"hello") + stored(b"")
    out.append(("one_byte_long", b"hell", z, [0, len(z)], False, False, [(LONG, 0)]))
    out.append(("one_byte_short", b"hello!", z, [0, len(z)], False, False, [(SHORT, 5)]))
    # an empty chunk with an empty stretch, and with the empty stored block alone
    out.append(("empty_chunk_empty_stretch", b"", b"", [0, 0], False, True, [(OK, 0)]))
    out.append(("empty_chunk_sync_only", b"", stored(b""), [0, 5], False, True, [(OK, 0)]))
    return out


def valid_cases():
    out = []
    for level in LEVELS:
        for n in SIZES:
            data = payload(n, 100 + level)
            for final in (False, True):
                z, off = zlib_stream(data, level, final)
                out.append(("zlib%d_n%d_%s" % (level, n, "final" if final else "sync"), data, z, off, final, True))
    return out


def _flip(z, bit):
    b = bytearray(z)
    b[bit >> 3] ^= 1 << (bit & 7)
    return bytes(b)


def damaged_cases():
    """Single-bit flips of one chunk's stretch, single staged bytes changed, a boundary entry moved by a byte -- on a
    level-9 stream of four chunks whose chunk 1 is a dynamic block with matches into chunk 0."""
    data = payload(3 * CHUNK + 1, 109)
    z, off = zlib_stream(data, 9, False)
    c = 1
    b0, b1 = off[c] * 8, off[c + 1] * 8
    assert (z[off[c]] >> 1) & 3 == 2, "chunk 1 should open with a dynamic block"
    bits = [b0] + list(range(b0, b0 + 64))
    body0, body1 = b0 + 64, b1 - 40
    bits += [body0 + (body1 - body0) * k // 32 + (k * 5) % 8 for k in range(32)]
    bits += list(range(b1 - 40, b1))
    out = []
    seen = set()
    for k, bit in enumerate(bits):
        if k and bit in seen:
            continue
        seen.add(bit)
        out.append(("flip_bit_%d%s" % (bit - b0, "_first" if k == 0 else ""), data, _flip(z, bit), off, False, False))
    for name, at in (("first", c * CHUNK), ("last", (c + 1) * CHUNK - 1), ("stream_last", len(data) - 1)):
        d = bytearray(data)
        d[at] ^= 0x01
        out.append(("staged_%s" % name, bytes(d), z, off, False, False))
    for k in (1, 2):
        for dlt in (-1, 1):
            o = list(off)
            o[k] += dlt
            out.append(("boundary_%d_%+d" % (k, dlt), data, z, o, False, False))
    return out


def all_cases():
    return [c[:6] for c in hand_built()] + valid_cases() + damaged_cases()


def zlib_accepts(data, z, z_off, c, final_chunk):
    """Does zlib decode chunk c's stretch to exactly the chunk, and does its stream end there?"""
    p0 = min(c * CHUNK, len(data))
    chunk = data[p0:p0 + CHUNK]
    stretch = z[z_off[c]:z_off[c + 1]] + (b"" if final_chunk else FINAL_EMPTY_STORED)
    front = data[max(0, p0 - 32768):p0]
    d = zlib.decompressobj(wbits=-15, zdict=front) if front else zlib.decompressobj(wbits=-15)
    try:
        got = d.decompress(stretch)
    except zlib.error:
        return False
    return got == chunk and d.eof and d.unused_data == b""
