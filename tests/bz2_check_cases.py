"""Block tables for the .bz2 producer's self-check (test_bz2_check_host.py on the CPU, test_gpu_bz2_check_edges.py on the GPU):
no asserts about the library here, only about the cases themselves.

A case is a Case: the compressed bytes `z`, the staged stream `data`, the stream's level, and a table of blocks -- z_beg / z_end
(bit offsets into z, MSB first), in_off / in_len (the block's piece of data) and crc (bzip2's CRC the host holds for the piece) --
and, where the case is made for one, the status every block must get (`expect`; None for the bit flips, of which only the
safety property is asked) and exact offsets (`offsets`: block -> offset).  block_ok(case, k) is the reference: libbz2, through
Python's bz2 module, decoding "BZh<level>" + the stretch's bits + the end-of-stream magic + the piece's CRC.

Good cases come from two writers: the producer's host model (snappy_amd/csrc/bzip2_enc_core.h through the harness's bc_encode)
over every input of bz2enc_cases at levels 1 and 9, and libbz2 itself (bz2.compress of each piece, the block's stretch found by
the install side's host scan)."""
import bz2
import ctypes
import functools

import bz2enc_cases as E
import hostbuild
import xz_cases as X

OK, BYTE, LENGTH, BLOCK, CAP, END, CRC, ORIGPTR, TABLE = range(9)
BLOCK_MAGIC, EOS_MAGIC = 0x314159265359, 0x177245385090
HEAD_BITS = 48 + 32 + 1 + 24  # magic, CRC, randomised, origPtr: the fixed part in front of the maps


class Case:
    def __init__(self, name, z, data, level, z_beg, z_end, in_off, in_len, crc, expect=None, kind="good", offsets=None):
        self.name, self.z, self.data, self.level = name, bytes(z), bytes(data), level
        self.z_beg, self.z_end, self.in_off, self.in_len, self.crc = list(z_beg), list(z_end), list(in_off), list(in_len), list(crc)
        self.expect, self.kind, self.offsets = expect, kind, dict(offsets or {})
        self.nb = len(self.z_beg)
        assert self.nb >= 1 and all(len(t) == self.nb for t in (self.z_end, self.in_off, self.in_len, self.crc))
        assert expect is None or len(expect) == self.nb

    def with_(self, name, kind, expect, offsets=None, **kw):
        f = dict(z=self.z, data=self.data, level=self.level, z_beg=self.z_beg, z_end=self.z_end, in_off=self.in_off, in_len=self.in_len, crc=self.crc)
        f.update(kw)
        return Case(name, expect=expect, kind=kind, offsets=offsets, **f)

    def one(self, k, name=None):
        """Block k alone, on the same buffers."""
        return Case(name or "%s[%d]" % (self.name, k), self.z, self.data, self.level, [self.z_beg[k]], [self.z_end[k]], [self.in_off[k]],
                    [self.in_len[k]], [self.crc[k]], None if self.expect is None else [self.expect[k]], self.kind,
                    {0: self.offsets[k]} if k in self.offsets else None)


# ---- bits -----------------------------------------------------------------------------------------------------------------------

def get_bits(z, bit, n):
    """The n bits at `bit` of z (MSB first), zeros past the end."""
    if n == 0:
        return 0
    a, b = bit // 8, (bit + n + 7) // 8
    chunk = z[a:b] + b"\0" * (b - a - len(z[a:b]))
    return (int.from_bytes(chunk, "big") >> ((b * 8) - bit - n)) & ((1 << n) - 1)


def put_bits(parts, pad_ones=False):
    """[(value, nbits)] one after another as bytes; the last byte's spare bits are zeros, or ones."""
    v = n = 0
    for val, k in parts:
        v, n = v << k | val, n + k
    pad = -n % 8
    v = v << pad | (((1 << pad) - 1) if pad_ones else 0)
    return v.to_bytes((n + pad) // 8, "big")


def flip_bit(z, bit):
    z = bytearray(z)
    z[bit // 8] ^= 0x80 >> (bit % 8)
    return bytes(z)


def set_field(z, bit, n, value):
    """z with the n bits at `bit` replaced by value."""
    old = get_bits(z, bit, n)
    out = bytearray(z)
    x = (old ^ value) & ((1 << n) - 1)
    for i in range(n):
        if x >> (n - 1 - i) & 1:
            out[(bit + i) // 8] ^= 0x80 >> ((bit + i) % 8)
    return bytes(out)


def block_ok(case, k):
    """libbz2's verdict on block k: does a stream of its stretch alone decode to exactly its piece?"""
    zb, ze = case.z_beg[k], case.z_end[k]
    if not (0 <= zb <= ze <= 8 * len(case.z)) or case.in_off[k] + case.in_len[k] > len(case.data):
        return False
    stream = b"BZh" + bytes([0x30 + case.level]) + put_bits([(get_bits(case.z, zb, ze - zb), ze - zb), (EOS_MAGIC, 48), (case.crc[k], 32)])
    try:
        out = bz2.decompress(stream)
    except (OSError, ValueError, EOFError):
        return False
    return out == case.data[case.in_off[k]:case.in_off[k] + case.in_len[k]]


def header_bits(z, bit):
    """How many bits the header of the (valid) block at `bit` takes: everything in front of the first coded symbol."""
    p = bit + HEAD_BITS
    used16 = get_bits(z, p, 16)
    p += 16
    nin = 0
    for i in range(16):
        if used16 >> (15 - i) & 1:
            nin += bin(get_bits(z, p, 16)).count("1")
            p += 16
    ngroups, nsel = get_bits(z, p, 3), get_bits(z, p + 3, 15)
    p += 18
    for _ in range(nsel):
        while get_bits(z, p, 1):
            p += 1
        p += 1
    for _ in range(ngroups):
        p += 5
        for _ in range(nin + 2):
            while get_bits(z, p, 1):
                p += 2
            p += 1
    return p - bit


# ---- the harness -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def load_harness():
    """tests/bz2_check_host_harness.cpp, loaded once a process with every prototype (it keeps no state between calls)."""
    L = hostbuild.shared("tests/bz2_check_host_harness.cpp")
    u64p, u32p, u8p, sz = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32), ctypes.c_char_p, ctypes.c_size_t
    L.bc_check.argtypes = [u8p, sz, u64p, u64p, u8p, sz, u64p, u64p, u32p, ctypes.c_uint32, sz, u32p]
    L.bc_check.restype = None
    L.bc_encode.argtypes = [u8p, sz, ctypes.c_uint32, ctypes.POINTER(sz)]
    L.bc_encode.restype = ctypes.c_void_p
    L.bc_free.argtypes = [ctypes.c_void_p]
    L.bc_scan.argtypes = [u8p, sz, u64p, sz]
    L.bc_scan.restype = ctypes.c_uint64
    L.bc_crc.argtypes = [u8p, sz]
    L.bc_crc.restype = ctypes.c_uint32
    L.bc_piece.argtypes = [ctypes.c_uint32]
    L.bc_piece.restype = ctypes.c_uint32
    L.bc_error_text.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_char_p, sz]
    L.bc_error_text.restype = sz
    return L


def host_verdicts(L, case):
    """[(status, offset)] a block, by the host model."""
    nb = case.nb
    v = (ctypes.c_uint32 * (2 * nb))()
    a64 = lambda t: (ctypes.c_uint64 * nb)(*t)
    L.bc_check(case.z, len(case.z), a64(case.z_beg), a64(case.z_end), case.data, len(case.data), a64(case.in_off), a64(case.in_len),
               (ctypes.c_uint32 * nb)(*case.crc), case.level, nb, v)
    return [(v[2 * k], v[2 * k + 1]) for k in range(nb)]


def model_stream(L, data, level):
    n = ctypes.c_size_t()
    p = L.bc_encode(data, len(data), level, ctypes.byref(n))
    try:
        return ctypes.string_at(p, n.value)
    finally:
        L.bc_free(p)


def stretches(L, stream):
    """[(z_beg, z_end)] of a whole stream's blocks: the starts by the install side's host scan, each block ending where the
    next begins, the last one at the end-of-stream magic (found from the stream's end: 48 + 32 bits and up to 7 of padding)."""
    cap = len(stream) // 32 + 64
    out = (ctypes.c_uint64 * cap)()
    n = L.bc_scan(stream, len(stream), out, cap)
    assert n <= cap
    starts = list(out[:n])
    eos = [len(stream) * 8 - 80 - pad for pad in range(8) if get_bits(stream, len(stream) * 8 - 80 - pad, 48) == EOS_MAGIC]
    assert len(eos) == 1 and starts == sorted(starts) and (not starts or starts[0] == 32)
    return list(zip(starts, starts[1:] + eos))


def stream_case(L, name, stream, data, level, piece_len):
    """A whole stream (BZh, blocks, footer) whose blocks hold piece_len bytes of data each, as one table."""
    st = stretches(L, stream)
    nb = (len(data) + piece_len - 1) // piece_len
    assert len(st) == nb, (name, len(st), nb)
    offs = [k * piece_len for k in range(nb)]
    lens = [min(piece_len, len(data) - o) for o in offs]
    crcs = [L.bc_crc(data[o:o + n], n) for o, n in zip(offs, lens)]
    return Case(name, stream, data, level, [a for a, _ in st], [b for _, b in st], offs, lens, crcs, [OK] * nb)


def model_case(L, name, data, level):
    return stream_case(L, "model_L%d_%s" % (level, name), model_stream(L, data, level), data, level, E.piece(level))


def libbz2_case(L, name, piece, level):
    """libbz2's own block for one piece (it must be one block: the piece's RLE1 form fits the level)."""
    return stream_case(L, "libbz2_L%d_%s" % (level, name), bz2.compress(piece, level), piece, level, max(len(piece), 1))


def aligned(case, k, a, carry=0xA5):
    """Block k of a case alone in a fresh buffer, its first bit at bit a (0..7) of a byte whose first a bits are the carry's, as a
    slot's first block lies behind the held-back byte; what follows the block in its last byte is ones."""
    n = case.z_end[k] - case.z_beg[k]
    z = put_bits([(carry >> (8 - a), a), (get_bits(case.z, case.z_beg[k], n), n)] if a else [(get_bits(case.z, case.z_beg[k], n), n)], pad_ones=True)
    return Case("%s[%d]@%d" % (case.name, k, a), z, case.data, case.level, [a], [a + n], [case.in_off[k]], [case.in_len[k]], [case.crc[k]], [OK])


def combine(name, cases, expect_from=None):
    """The cases' buffers one after another and one table of all their blocks (same level)."""
    z, data, zb, ze, io, il, crc, exp, offs = b"", b"", [], [], [], [], [], [], {}
    for c in cases:
        assert c.level == cases[0].level and c.expect is not None
        for k in range(c.nb):
            if k in c.offsets:
                offs[len(zb) + k] = c.offsets[k]
        zb += [x + 8 * len(z) for x in c.z_beg]
        ze += [x + 8 * len(z) for x in c.z_end]
        io += [x + len(data) for x in c.in_off]
        il += c.in_len
        crc += c.crc
        exp += c.expect
        z += c.z
        data += c.data
    return Case(name, z, data, cases[0].level, zb, ze, io, il, crc, exp, "combined", offs)


def no_runs(n, seed):
    """n random bytes without four equal in a row: RLE1 leaves them n bytes."""
    out = bytearray(X.rnd(n, seed=seed))
    for i in range(3, n):
        if out[i] == out[i - 1] == out[i - 2] == out[i - 3]:
            out[i] ^= 0x55
    return bytes(out)


# ---- good cases ----------------------------------------------------------------------------------------------------------------

def edge_inputs():
    """(name, piece): where the RLE1 chunk count and size change, runs at a piece's ends, the full level-1 piece."""
    c = [("rle_%d" % n, no_runs(n, 70 + n % 13)) for n in (1, 64, 65, 1024 * 64 + 1)]
    c.append(("piece_exact", X.text(E.PIECE, seed=77)))
    for k in (4, 5, 259, 260):
        c.append(("run_%d_first" % k, b"r" * k + X.text(3000, seed=78)))
        c.append(("run_%d_last" % k, X.text(3000, seed=79) + b"r" * k))
    return c


def good_cases(L, big=True):
    """Every accepted case.  big=False leaves out the level-9 model streams of the large inputs (the GPU suite's budget)."""
    out = []
    for name, data in E.cases():
        if not data:
            continue
        out.append(model_case(L, name, data, 1))
        if big:
            out.append(model_case(L, name, data, 9))
        for i in range(0, len(data), E.PIECE):  # libbz2's own block for each piece
            out.append(libbz2_case(L, "%s_p%d" % (name, i // E.PIECE), data[i:i + E.PIECE], 1))
    for name, piece in edge_inputs():
        out.append(model_case(L, name, piece, 1))
        out.append(libbz2_case(L, name, piece, 1))
    small = model_case(L, "small", X.text(3000, seed=80), 1)
    lib_small = libbz2_case(L, "small", X.text(3000, seed=80), 1)
    for a in range(8):
        out.append(aligned(small, 0, a))
        out.append(aligned(lib_small, 0, a))
    two = model_case(L, "two_blocks", X.text(E.PIECE + 1234, seed=81), 1)
    out += [aligned(two, 1, a) for a in range(8)]
    out += periodic_cases(L)
    return out


def periodic_cases(L):
    """A block periodic after RLE1, u^k: the k rotations that equal rotation 0 form a tie group of k consecutive ranks, and the
    block with ANY of them as origPtr decodes to the same bytes.  The producer writes the group's first (equal rotations sort
    by start index)."""
    out = []
    for name, u, k in (("u2", no_runs(500, 90), 2), ("ab1000", b"ab", 1000)):
        base = model_case(L, "periodic_" + name, u * k, 1)
        op = get_bits(base.z, base.z_beg[0] + 81, 24)
        for t in range(k):
            out.append(base.with_("%s_op+%d" % (base.name, t), "good", [OK], z=set_field(base.z, base.z_beg[0] + 81, 24, op + t)))
    return out


# ---- damaged cases ---------------------------------------------------------------------------------------------------------------

def damaged_cases(L):
    out = []
    base = model_case(L, "dmg", X.text(3000, seed=82), 1)
    zb, ze, n = base.z_beg[0], base.z_end[0], len(base.data)
    for at in (0, n // 2, n - 1):  # a staged byte changed: the offset must be exact
        d = bytearray(base.data)
        d[at] ^= 1
        out.append(base.with_("staged_%d" % at, "staged", [BYTE], {0: at}, data=bytes(d)))
    out.append(base.with_("in_len-1", "length", [LENGTH], {0: n - 1}, in_len=[n - 1]))
    out.append(base.with_("in_len+1", "length", [LENGTH], {0: n}, data=base.data + b"\0", in_len=[n + 1]))
    out.append(base.with_("crc", "crc", [CRC], {0: 0}, crc=[base.crc[0] ^ 1]))
    out.append(base.with_("z_end+1", "end", [END], {0: ze - zb}, z=base.z + b"\0", z_end=[ze + 1]))
    out.append(base.with_("z_end-1", "end", [END], {0: ze - zb}, z_end=[ze - 1]))
    out.append(base.with_("z_beg+1", "block", [BLOCK], {0: 4}, z_beg=[zb + 1]))
    out.append(base.with_("z_beg-1", "block", [BLOCK], {0: 4}, z_beg=[zb - 1]))
    op = get_bits(base.z, zb + 81, 24)
    nsym = 3000  # (prose without runs of four: RLE1 leaves it as it is)
    out.append(base.with_("origptr_n", "origptr", [ORIGPTR], {0: nsym}, z=set_field(base.z, zb + 81, 24, nsym)))
    out.append(base.with_("origptr_max", "origptr", [ORIGPTR], {0: 0xffffff}, z=set_field(base.z, zb + 81, 24, 0xffffff)))
    out.append(base.with_("origptr_other", "origptr_other", [BYTE], None, z=set_field(base.z, zb + 81, 24, (op + 1) % nsym)))
    out.append(base.with_("randomised", "block", [BLOCK], {0: 4}, z=flip_bit(base.z, zb + 80)))
    out.append(base.with_("truncated", "block", [BLOCK], {0: 2}, z=base.z[:ze // 8 - 12], z_end=[8 * (ze // 8 - 12)]))
    big = model_case(L, "over_level", X.text(150000, seed=83), 9)  # one level-9 block of 150 000 symbols, held against level 1
    out.append(big.with_("level_lowered", "cap", [CAP], {0: 100000}, level=1))
    out.append(base.with_("z_end_past", "table", [TABLE], {0: 0}, z_end=[8 * len(base.z) + 1]))
    out.append(base.with_("z_reversed", "table", [TABLE], {0: 0}, z_beg=[ze], z_end=[zb]))
    out.append(base.with_("in_past", "table", [TABLE], {0: 0}, in_off=[1]))
    out.append(base.with_("in_off_past", "table", [TABLE], {0: 0}, in_off=[n + 1], in_len=[0]))
    out.append(base.with_("z_huge", "table", [TABLE], {0: 0}, z_beg=[2 ** 64 - 2], z_end=[2 ** 64 - 1]))
    # every single-bit flip of one small block's header, and 32 spread over its body: the safety property alone
    tiny = model_case(L, "tiny", b"hello hello hello world, " * 3, 1)
    tb, te = tiny.z_beg[0], tiny.z_end[0]
    hb = header_bits(tiny.z, tb)
    assert HEAD_BITS + 16 < hb < te - tb
    for i in range(hb):
        out.append(tiny.with_("flip_h%d" % i, "flip", None, z=flip_bit(tiny.z, tb + i)))
    body = te - tb - hb
    for i in range(32):
        out.append(tiny.with_("flip_b%d" % i, "flip", None, z=flip_bit(tiny.z, tb + hb + i * body // 32)))
    return out
