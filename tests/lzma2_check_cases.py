"""Chunk tables for the .xz producer's self-check (test_lzma2_check_host.py on the CPU, test_gpu_lzma2_check_edges.py on the
GPU): no asserts about the library here, only about the cases themselves.

A case is a Case: the staged stream `data`, the Block size, the compressed bytes `z`, the two tables z_beg / z_end (a
stretch a chunk of 65 536 staged bytes) and, where the case is made for one, the status every chunk must get (`expect`; None
for the bit flips, of which only the safety property is asked).  block_ok(case, k) is the reference: liblzma, through Python's
lzma module, decoding the concatenated stretches of Block k's chunks as raw LZMA2.

Good cases come from three writers: the producer's host model (snappy_amd/csrc/xz_enc_core.h through the harness's lc_encode)
over every input of xzenc_cases, liblzma itself (each 64 KiB piece compressed alone and re-labelled as xz_cases.join_raw
does), and a symbol coder of this file's own on xz_cases._RangeEncoder for the chunks neither of them writes.  Every good
case is decoded by liblzma before it is returned.  The Block size is 128 KiB unless the case says otherwise."""
import ctypes
import functools
import lzma

import hostbuild
import xz_cases as X
import xzenc_cases as E

CHUNK = 65536
B = 128 * 1024
OK, LITERAL, MATCH, DISTANCE, BAD, LONG, USIZE, END, TABLE = range(9)
FILL = 0xAA  # what stands where the host would write Block headers, padding and Checks


class Case:
    def __init__(self, name, data, bs, z, z_beg, z_end, expect=None, kind="good"):
        self.name, self.data, self.bs, self.z = name, bytes(data), bs, bytes(z)
        self.z_beg, self.z_end, self.expect, self.kind = list(z_beg), list(z_end), expect, kind
        self.nch = (len(self.data) + CHUNK - 1) // CHUNK
        assert self.nch == len(self.z_beg) == len(self.z_end) and self.nch >= 1
        assert expect is None or len(expect) == self.nch

    def blocks(self):
        """[(first chunk, chunks, staged bytes)] a Block."""
        cpb = self.bs // CHUNK
        return [(k * cpb, min(cpb, self.nch - k * cpb), self.data[k * self.bs:(k + 1) * self.bs]) for k in range((len(self.data) + self.bs - 1) // self.bs)]

    def with_(self, name, kind, expect, data=None, z=None, z_beg=None, z_end=None):
        return Case(name, self.data if data is None else data, self.bs, self.z if z is None else z, self.z_beg if z_beg is None else z_beg,
                    self.z_end if z_end is None else z_end, expect, kind)


def block_ok(case, k):
    """liblzma's verdict on Block k: do its chunks' stretches, one after another, decode to exactly the Block's staged bytes
    and end there?"""
    c0, cn, staged = case.blocks()[k]
    raw = b""
    for c in range(c0, c0 + cn):
        if not (0 <= case.z_beg[c] <= case.z_end[c] <= len(case.z)):
            return False
        raw += case.z[case.z_beg[c]:case.z_end[c]]
    d = lzma.LZMADecompressor(lzma.FORMAT_RAW, filters=[dict(id=lzma.FILTER_LZMA2, dict_size=max(case.bs, 4096))])
    try:
        out = d.decompress(raw)
    except lzma.LZMAError:
        return False
    return d.eof and not d.unused_data and out == staged


# ---- the harness -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def load_harness():
    """tests/lzma2_check_host_harness.cpp, loaded once a process with every prototype (it keeps no state between calls)."""
    L = hostbuild.shared("tests/lzma2_check_host_harness.cpp")
    u64p, u8p = ctypes.POINTER(ctypes.c_uint64), ctypes.c_char_p
    L.lc_check.argtypes = [u8p, ctypes.c_size_t, ctypes.c_uint64, u8p, ctypes.c_size_t, u64p, u64p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32)]
    L.lc_check.restype = None
    L.lc_encode.argtypes = [u8p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_size_t, u64p, u64p]
    L.lc_encode.restype = ctypes.c_int64
    L.lc_error_text.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t]
    L.lc_error_text.restype = ctypes.c_size_t
    return L


def host_verdicts(L, case):
    """[(status, offset)] a chunk, by the host walker."""
    v = (ctypes.c_uint32 * (2 * case.nch))()
    beg = (ctypes.c_uint64 * case.nch)(*case.z_beg)
    end = (ctypes.c_uint64 * case.nch)(*case.z_end)
    L.lc_check(case.data, len(case.data), case.bs, case.z, len(case.z), beg, end, case.nch, v)
    return [(v[2 * c], v[2 * c + 1]) for c in range(case.nch)]


def model_case(L, name, data, bs):
    """The producer's host model over data: what lzma2_concat_kernel leaves in the slot's output buffer, over FILL."""
    bs = bs or 1 << 20
    nch = (len(data) + CHUNK - 1) // CHUNK
    cap = len(data) + nch * 64 + 64
    out = ctypes.create_string_buffer(bytes([FILL]) * cap, cap)
    beg, end = (ctypes.c_uint64 * nch)(), (ctypes.c_uint64 * nch)()
    total = L.lc_encode(data, len(data), bs, out, cap, beg, end)
    assert total > 0, name
    return Case("model_" + name, data, bs, out.raw[:total], list(beg), list(end), [OK] * nch)


# ---- a symbol coder for one chunk ------------------------------------------------------------------------------------------------

class _RC(X._RangeEncoder):
    def tree_rev(self, base, nbits, value):
        m = 1
        for i in range(nbits):
            b = value >> i & 1
            self.bit(base + m, b)
            m = m << 1 | b

    def direct(self, value, nbits):
        for i in range(nbits - 1, -1, -1):
            self.range >>= 1
            if value >> i & 1:
                self.low += self.range
            while self.range < 1 << 24:
                self.range = (self.range << 8) & 0xFFFFFFFF
                self._shift_low()


class ChunkCoder:
    """The LZMA symbols of one chunk (lc=3 lp=0 pb=2, state reset), written one by one.  blk: the Block's bytes, the
    dictionary and the contexts; pos: where the chunk begins in it.  The symbols are written as asked, whether the Block's
    bytes bear them out or not (the damaged cases ask for some that they do not).  Probability offsets as in
    xz_cases.run_chunk; SpecPos at 688, Align at 802, IsRepG1 216, IsRepG2 228."""

    def __init__(self, blk, pos):
        self.rc, self.blk, self.start, self.pos, self.state, self.reps = _RC(), blk, pos, pos, 0, [0, 0, 0, 0]

    def literal(self, byte=None):
        rc, pos = self.rc, self.pos
        b = self.blk[pos] if byte is None else byte
        rc.bit((self.state << 4) + (pos & 3), 0)
        base = 1846 + 0x300 * ((self.blk[pos - 1] if pos else 0) >> 5)
        if self.state < 7:
            rc.tree(base, 8, b)
        else:
            mb, offs, sym = self.blk[pos - self.reps[0] - 1], 0x100, 1
            for i in range(7, -1, -1):
                mb <<= 1
                mbit = mb & offs
                bit = b >> i & 1
                rc.bit(base + offs + mbit + sym, bit)
                sym = sym << 1 | bit
                offs &= mbit if bit else ~mbit
        self.state = 0 if self.state < 4 else self.state - 3 if self.state < 10 else self.state - 6
        self.pos += 1
        return self

    def literals(self, n):
        for _ in range(n):
            self.literal()
        return self

    def _len(self, base, ln, ps):
        rc = self.rc
        if ln < 10:
            rc.bit(base, 0)
            rc.tree(base + 2 + (ps << 3), 3, ln - 2)
        elif ln < 18:
            rc.bit(base, 1)
            rc.bit(base + 1, 0)
            rc.tree(base + 130 + (ps << 3), 3, ln - 10)
        else:
            rc.bit(base, 1)
            rc.bit(base + 1, 1)
            rc.tree(base + 258, 8, ln - 18)

    def match(self, dist, ln):
        rc, ps, d1 = self.rc, self.pos & 3, dist - 1
        rc.bit((self.state << 4) + ps, 1)
        rc.bit(192 + self.state, 0)
        self._len(818, ln, ps)
        self.state = 7 if self.state < 7 else 10
        slot = d1 if d1 < 4 else 2 * (d1.bit_length() - 1) + (d1 >> (d1.bit_length() - 2) & 1)
        rc.tree(432 + (min(ln - 2, 3) << 6), 6, slot)
        if slot >= 4:
            nb = (slot >> 1) - 1
            base = (2 | (slot & 1)) << nb
            if slot < 14:
                rc.tree_rev(688 + base - slot - 1, nb, d1 - base)
            else:
                rc.direct((d1 - base) >> 4, nb - 4)
                rc.tree_rev(802, 4, (d1 - base) & 15)
        self.reps = [d1] + self.reps[:3]
        self.pos += ln
        return self

    def rep(self, k, ln):
        rc, ps = self.rc, self.pos & 3
        rc.bit((self.state << 4) + ps, 1)
        rc.bit(192 + self.state, 1)
        if k == 0:
            rc.bit(204 + self.state, 0)
            rc.bit(240 + (self.state << 4) + ps, 1)
        else:
            rc.bit(204 + self.state, 1)
            if k == 1:
                rc.bit(216 + self.state, 0)
            else:
                rc.bit(216 + self.state, 1)
                rc.bit(228 + self.state, k - 2)
            self.reps.insert(0, self.reps.pop(k))
        self._len(1332, ln, ps)
        self.state = 8 if self.state < 7 else 11
        self.pos += ln
        return self

    def short_rep(self):
        rc, ps = self.rc, self.pos & 3
        rc.bit((self.state << 4) + ps, 1)
        rc.bit(192 + self.state, 1)
        rc.bit(204 + self.state, 0)
        rc.bit(240 + (self.state << 4) + ps, 0)
        self.state = 9 if self.state < 7 else 11
        self.pos += 1
        return self

    def chunk(self, first, usize=None):
        """The chunk as LZMA2 writes it: 0xE0 / 0xC0, both sizes, 0x5D, the coder's bytes."""
        body = self.rc.finish()
        n = (self.pos - self.start if usize is None else usize) - 1
        assert 0 <= n < 1 << 21 and 5 <= len(body) <= 1 << 16
        return bytes([(0xE0 if first else 0xC0) | n >> 16, n >> 8 & 0xFF, n & 0xFF, (len(body) - 1) >> 8, (len(body) - 1) & 0xFF, 0x5D]) + body


def stored(piece, first):
    assert 1 <= len(piece) <= CHUNK
    return bytes([1 if first else 2, (len(piece) - 1) >> 8, (len(piece) - 1) & 0xFF]) + piece


def assemble(name, data, bs, chunks, expect=None, kind="good", head=12, gap=16):
    """The chunks (header and body each) in place as the producer lays them out: FILL where a Block's header stands, the
    Block's chunks back to back, its end byte, FILL for padding and Check."""
    cpb = bs // CHUNK
    z, beg, end = bytearray([FILL] * head), [], []
    for c, ch in enumerate(chunks):
        beg.append(len(z))
        z += ch
        last = (c + 1) % cpb == 0 or c + 1 == len(chunks)
        if last:
            z.append(0)
        end.append(len(z))
        if last:
            z += bytes([FILL] * gap)
    return Case(name, data, bs, z, beg, end, [OK] * len(chunks) if expect is None else expect, kind)


# ---- good cases --------------------------------------------------------------------------------------------------------------------

def _liblzma_chunk(piece, preset, first):
    raw = lzma.compress(piece, format=lzma.FORMAT_RAW, filters=[dict(id=lzma.FILTER_LZMA2, preset=preset, dict_size=1 << 20)])
    ctl = raw[0]
    if ctl >= 0x80:
        assert ctl >= 0xE0 and raw[5] == 0x5D
        n = 6 + (raw[3] << 8 | raw[4]) + 1
        ch = bytes([(0xE0 if first else 0xC0) | ctl & 0x1F]) + raw[1:n]
    else:
        assert ctl == 1
        n = 3 + (raw[1] << 8 | raw[2]) + 1
        ch = bytes([1 if first else 2]) + raw[1:n]
    assert len(raw) == n + 1 and raw[n] == 0, "one chunk a piece"
    return ch


def liblzma_cases():
    """Each 64 KiB piece compressed alone by liblzma; a piece that another follows in its Block ends in a zero byte, so that
    the literal context at the next chunk's first byte is the one its encoder saw (xz_cases.join_raw)."""
    def z0(p):
        return p[:-1] + b"\0"
    out = []
    # (liblzma ends a chunk once its coder has filled 64 KiB less a margin, so 64 KiB it cannot compress leave it in two chunks:
    # the incompressible pieces are a stream's last, shorter ones)
    layouts = (("text_text", [z0(X.text(CHUNK, 201)), X.text(CHUNK, 202)]),
               ("text_rnd", [z0(X.text(CHUNK, 203)), X.rnd(30000, 204)]),
               ("text_text_rnd", [z0(X.text(CHUNK, 205)), X.text(CHUNK, 206), X.rnd(50000, 207)]),
               ("text_text_text_tail", [z0(X.text(CHUNK, 208)), X.text(CHUNK, 209), z0(X.text(CHUNK, 210)), X.text(1000, 211)]))
    for preset in (0, 6, 9 | lzma.PRESET_EXTREME):
        for lname, pieces in layouts:
            chunks = [_liblzma_chunk(p, preset, c % (B // CHUNK) == 0) for c, p in enumerate(pieces)]
            out.append(assemble("liblzma_p%d_%s" % (preset & 15, lname), b"".join(pieces), B, chunks))
    assert any(c.z[c.z_beg[1]] == 2 for c in out) and any(c.nch > 2 and c.z[c.z_beg[2]] == 1 for c in out)  # stored, later and first
    return out


def _front(seed, tail=0x41):
    """A full chunk of text whose last byte is known."""
    return X.text(CHUNK - 1, seed) + bytes([tail])


def hand_cases():
    out = []
    # a match in chunk 1 at distance exactly the bytes in front of it in the Block
    f = _front(301)
    data = f + b"hello" + f[:8] + b"zz"
    c1 = ChunkCoder(data, CHUNK).literals(5).match(CHUNK + 5, 8).literals(2)
    out.append(assemble("dist_is_front", data, B, [stored(f, True), c1.chunk(False)]))
    # rep0 - rep3 and a short rep at a later chunk's first position (the reps are all distance 1 after the state reset)
    for k in range(4):
        data = f + b"A" * 6 + b"xy"
        c1 = ChunkCoder(data, CHUNK).rep(k, 6).literals(2)
        out.append(assemble("rep%d_first" % k, data, B, [stored(f, True), c1.chunk(False)]))
    data = f + b"A" + b"xy"
    out.append(assemble("short_rep_first", data, B, [stored(f, True), ChunkCoder(data, CHUNK).short_rep().literals(2).chunk(False)]))
    # a matched literal whose match byte lies in the previous chunk
    data = f + f[CHUNK - 10:CHUNK - 8] + b"Q" + b"tail"
    assert data[CHUNK + 2 - 10] != data[CHUNK + 2]
    c1 = ChunkCoder(data, CHUNK).match(10, 2).literals(5)
    out.append(assemble("matched_literal_prev_chunk", data, B, [stored(f, True), c1.chunk(False)]))
    # a length-273 match ending exactly at the chunk's end: a short last chunk, and a full one that another follows
    data = f + b"abc" + f[100:373]
    c1 = ChunkCoder(data, CHUNK).literals(3).match(CHUNK + 3 - 100, 273)
    out.append(assemble("len273_ends_chunk", data, B, [stored(f, True), c1.chunk(False)]))
    g = X.text(CHUNK - 273, 302) + f[500:773]
    data = f + g + b"next"
    c1 = ChunkCoder(data, CHUNK).literals(CHUNK - 273).match(2 * CHUNK - 273 - 500, 273)
    c2 = ChunkCoder(data[2 * CHUNK:], 0).literals(4)
    out.append(assemble("len273_ends_full_chunk", data, B, [stored(f, True), c1.chunk(False), c2.chunk(True)]))
    # a 1-byte last chunk, as LZMA and stored
    data = f + b"k"
    out.append(assemble("one_byte_lzma", data, B, [stored(f, True), ChunkCoder(data, CHUNK).literal().chunk(False)]))
    out.append(assemble("one_byte_stored", data, B, [stored(f, True), stored(b"k", False)]))
    # 64 KiB Blocks: every chunk the first and the last of its Block
    g = _front(303, 0x42)
    data = f + g + b"abcabcabc"
    c2 = ChunkCoder(data[2 * CHUNK:], 0).literals(3).match(3, 6)
    out.append(assemble("blocks_64k", data, CHUNK, [stored(f, True), stored(g, True), c2.chunk(True)]))
    return out


def good_cases(L):
    out = [model_case(L, name, data, bs) for name, data, bs in E.cases() if len(data)]
    out += liblzma_cases() + hand_cases()
    for c in out:
        for k in range(len(c.blocks())):
            assert block_ok(c, k), (c.name, k)
    return out


# ---- damaged cases -----------------------------------------------------------------------------------------------------------------

def _flip(b, at, bit):
    b = bytearray(b)
    b[at] ^= bit
    return bytes(b)


def _hand_base():
    """Block 0: a stored chunk and a hand-coded one -- 4 literals, a match of 20 from offset 100 of chunk 0, 2 literals, a
    match of 5 from 6 back, 3 literals: 34 bytes.  What every symbol covers is known."""
    f = _front(401)
    tail = b"wxyz" + f[100:120] + b"pq"
    tail += tail[-6:-1] + b"end"
    data = f + tail
    c1 = ChunkCoder(data, CHUNK).literals(4).match(CHUNK + 4 - 100, 20).literals(2).match(6, 5).literals(3)
    return assemble("hand_base", data, B, [stored(f, True), c1.chunk(False)]), f


def damaged_cases(L):
    """Cases with `expect` (kinds staged, table, end_byte, distance, length, control, props, header) and the bit flips
    (kind flip, expect None)."""
    out = []
    # the bit flips: chunk 1 of the model's three chunks of text (an LZMA chunk, a later one, its Block's last)
    base = model_case(L, "flip_base", X.text(2 * CHUNK + 3000, 400), B)
    b1, e1 = base.z_beg[1], base.z_end[1]
    assert base.z[b1] == 0xC0 and base.z[e1 - 1] == 0 and e1 - b1 > 2000
    spots = [(b1 + i, 1 << bit) for i in range(11) for bit in range(8)]
    spots += [(b1 + 11 + (e1 - b1 - 16) * k // 24, 1 << (k % 8)) for k in range(24)]
    spots += [(e1 - 1 - i, bit) for i in range(1, 5) for bit in (0x01, 0x80)]
    for at, bit in spots:
        out.append(base.with_("flip_%d_%02x" % (at - b1, bit), "flip", None, z=_flip(base.z, at, bit)))
    hb, f = _hand_base()
    b1, e1 = hb.z_beg[1], hb.z_end[1]
    # a staged byte changed under a literal, inside a match body, and in the PREVIOUS chunk under a match's source (chunk 0's
    # stored copy changed with it: chunk 0 is what it was made from, chunk 1 is not)
    out.append(hb.with_("staged_under_literal", "staged", [OK, LITERAL], data=_flip(hb.data, CHUNK + 1, 1)))
    out[-1].offsets = {1: 1}
    out.append(hb.with_("staged_in_match_body", "staged", [OK, MATCH], data=_flip(hb.data, CHUNK + 4 + 7, 1)))
    out[-1].offsets = {1: 11}
    out.append(hb.with_("staged_under_match_source", "staged", [OK, MATCH], data=_flip(hb.data, 103, 1), z=_flip(hb.z, hb.z_beg[0] + 3 + 103, 1)))
    out[-1].offsets = {1: 7}
    out.append(hb.with_("staged_in_stored", "staged", [LITERAL, OK], data=_flip(hb.data, 70, 1)))  # (not under chunk 1's match: 100..120)
    out[-1].offsets = {0: 70}
    # z_beg / z_end moved by one.  In front of chunk 1 lies chunk 0's last byte, 0x41: no control byte; behind its control byte
    # the size byte 0x00: an end byte where a chunk must stand
    assert hb.z[b1 - 1] == 0x41 and hb.z[b1 + 1] == 0
    out.append(hb.with_("z_beg_minus_1", "table", [OK, BAD], z_beg=[hb.z_beg[0], b1 - 1]))
    out.append(hb.with_("z_beg_plus_1", "table", [OK, BAD], z_beg=[hb.z_beg[0], b1 + 1]))
    out.append(hb.with_("z_end_minus_1", "table", [OK, END], z_end=[hb.z_end[0], e1 - 1]))
    out.append(hb.with_("z_end_plus_1", "table", [OK, END], z_end=[hb.z_end[0], e1 + 1]))
    out.append(hb.with_("z_end0_minus_1", "table", [END, OK], z_end=[hb.z_end[0] - 1, e1]))
    out.append(hb.with_("z_end0_plus_1", "table", [END, OK], z_end=[hb.z_end[0] + 1, e1]))
    # entries past n_z, and an end in front of its beginning
    n_z = len(hb.z)
    out.append(hb.with_("z_end_past_n_z", "table", [OK, TABLE], z_end=[hb.z_end[0], n_z + 1]))
    out.append(hb.with_("z_both_past_n_z", "table", [OK, TABLE], z_beg=[hb.z_beg[0], n_z + 5], z_end=[hb.z_end[0], n_z + 50]))
    out.append(hb.with_("z_beg_far_past", "table", [TABLE, OK], z_beg=[1 << 40, b1], z_end=[(1 << 40) + 10, e1]))
    out.append(hb.with_("z_end_before_beg", "table", [OK, TABLE], z_beg=[hb.z_beg[0], e1], z_end=[hb.z_end[0], b1]))
    # the end byte: missing (FILL stands there), non-zero, and given to a chunk that is not its Block's last
    out.append(hb.with_("end_byte_missing", "end_byte", [OK, END], z=hb.z[:e1 - 1] + hb.z[e1:], z_end=[hb.z_end[0], e1 - 1]))
    out.append(hb.with_("end_byte_fill", "end_byte", [OK, END], z=hb.z[:e1 - 1] + hb.z[e1:]))  # (the stretch as long as it should be)
    out.append(hb.with_("end_byte_nonzero", "end_byte", [OK, END], z=_flip(hb.z, e1 - 1, 1)))
    z = hb.z[:b1] + b"\0" + hb.z[b1:]
    out.append(hb.with_("end_byte_not_last", "end_byte", [END, OK], z=z, z_beg=[hb.z_beg[0], b1 + 1], z_end=[hb.z_end[0] + 1, e1 + 1]))
    # a distance one beyond the bound: in a later chunk and in a Block's first
    data = f + b"wxyz" + b"?" * 8 + b"pq"
    c1 = ChunkCoder(data, CHUNK).literals(4).match(CHUNK + 4 + 1, 8).literals(2)
    out.append(assemble("distance_beyond_later", data, B, [stored(f, True), c1.chunk(False)], [OK, DISTANCE], "distance"))
    out[-1].offsets = {1: 4}
    c1 = ChunkCoder(data, CHUNK).literals(4).match(CHUNK + 4, 8).literals(2)  # (the bound itself, over bytes that differ)
    assert data[:8] != data[CHUNK + 4:CHUNK + 12]
    out.append(assemble("distance_at_bound_differs", data, B, [stored(f, True), c1.chunk(False)], [OK, MATCH], "distance"))
    data = b"abc" + b"abcabc" + b"zz"
    c0 = ChunkCoder(data, 0).literals(3).match(4, 6).literals(2)
    out.append(assemble("distance_beyond_first", data, B, [c0.chunk(True)], [DISTANCE], "distance"))
    out[-1].offsets = {0: 3}
    c0 = ChunkCoder(data, 0).rep(0, 6)
    out.append(assemble("rep_before_any_byte", data[:6], B, [c0.chunk(True)], [DISTANCE], "distance"))
    data64 = f + b"abc" + b"abcabc"  # with 64 KiB Blocks chunk 1 begins a Block: the bytes in front belong to another
    c1 = ChunkCoder(data64[CHUNK:], 0).literals(3).match(4, 6)
    out.append(assemble("distance_into_previous_block", data64, CHUNK, [stored(f, True), c1.chunk(True)], [OK, DISTANCE], "distance"))
    # a match one longer than the chunk's remainder
    data = f + b"wxyz" + f[100:120]
    c1 = ChunkCoder(data, CHUNK).literals(4).match(CHUNK + 4 - 100, 21)
    out.append(assemble("match_past_chunk", data, B, [stored(f, True), c1.chunk(False, usize=24)], [OK, LONG], "length"))
    out[-1].offsets = {1: 4}
    g = X.text(CHUNK - 20, 402) + f[100:120]
    data = f + g + f[120:121] + b"more"
    c1 = ChunkCoder(data, CHUNK).literals(CHUNK - 20).match(2 * CHUNK - 20 - 100, 21)  # (the bytes bear it out: it is the chunk that ends)
    c2 = ChunkCoder(data[2 * CHUNK:], 0).literals(5)
    out.append(assemble("match_into_next_chunk", data, B, [stored(f, True), c1.chunk(False, usize=CHUNK), c2.chunk(True)], [OK, LONG, OK], "length"))
    # controls, properties, header sizes, the first range coder byte
    for ctl in (0x80, 0xA0, 0xE0):
        out.append(hb.with_("control_%02x_later" % ctl, "control", [OK, BAD], z=hb.z[:b1] + bytes([ctl]) + hb.z[b1 + 1:]))
    z0 = hb.z_beg[0]
    out.append(hb.with_("control_02_first", "control", [BAD, OK], z=hb.z[:z0] + b"\x02" + hb.z[z0 + 1:]))
    out.append(hb.with_("control_01_later", "control", [OK, BAD], z=hb.z[:b1] + b"\x01" + hb.z[b1 + 1:]))
    out.append(hb.with_("control_03", "control", [BAD, OK], z=hb.z[:z0] + b"\x03" + hb.z[z0 + 1:]))
    out.append(hb.with_("props_5e", "props", [OK, BAD], z=_flip(hb.z, b1 + 5, 0x5D ^ 0x5E)))
    out.append(hb.with_("usize_minus_1", "header", [OK, USIZE], z=_flip(hb.z, b1 + 2, 1)))
    out.append(hb.with_("csize_plus_1", "header", [OK, END], z=hb.z[:b1 + 4] + bytes([hb.z[b1 + 4] + 1]) + hb.z[b1 + 5:]))
    out.append(hb.with_("rc_first_byte", "header", [OK, BAD], z=_flip(hb.z, b1 + 6, 0x40)))
    # the coder's end: the same symbols with one more zero byte of body (csize says so: the sizes meet, the coder does not)
    ch = hb.z[b1:e1 - 1]
    ch = ch[:3] + bytes([(len(ch) - 6) >> 8, (len(ch) - 6) & 0xFF]) + ch[5:] + b"\0"
    c = assemble("body_one_longer", hb.data, B, [stored(f, True), ch], [OK, END], "header")
    out.append(c)
    for c in out:
        assert c.kind == "flip" or any(not block_ok(c, k) for k in range(len(c.blocks()))), c.name  # liblzma refuses each too
    return out
