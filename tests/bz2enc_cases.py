"""Inputs of the .bz2 writer's tests (test_bz2enc_host.py on the CPU, test_gpu_bz2enc.py on the GPU): no asserts about the
library here.  Built for level 1, where a block takes PIECE = 79 872 bytes of input, so that every case is tens to a few
hundred KiB; cases() gives (name, data) pairs, big_cases() the few that need a level above 1 to be one block."""
import functools
import random

import xz_cases as X


def piece(level):
    """bzenc_piece: input bytes of a block."""
    return (100000 * level - 19) * 4 // 5 // 512 * 512


PIECE = piece(1)
assert PIECE == 79872 and piece(9) == 719872


def runs_of_four(n):
    """Runs of exactly four of alternating bytes: RLE1 makes five of every four."""
    return (b"aaaabbbb" * (n // 8 + 1))[:n]


def all_bytes(n, seed=11):
    r = random.Random(seed)
    return bytes(range(256)) + bytes(r.randrange(256) for _ in range(n - 256))


def one_row(n, row=5, seed=12):
    """Byte values of one 16-value row of the symbol map only (no byte twice in a row: RLE1 adds no count byte)."""
    r = random.Random(seed)
    out, last = bytearray(), 0
    for _ in range(n):
        last = (last + 1 + r.randrange(15)) % 16
        out.append(row * 16 + last)
    return bytes(out)


def sorted_runs(seed=13):
    """Long runs in the BWT's last column: ab x m has the last column b^m a^m, a zero run of m - 1."""
    out = []
    for k in range(1, 16):  # (2^16 needs more than a level-1 piece: big_cases)
        for d in (-1, 0, 1):
            out.append(("zero_run_2^%d%+d" % (k, d), b"ab" * ((1 << k) + d + 1)))
    return out


def sources_like(n, seed=15):
    """Program text: indented lines of a few identifiers, keywords and punctuation, blocks that open and close.  (xz_cases
    has generators for prose-like text, random bytes and random bytes with copies, none for sources.)"""
    r = random.Random(seed)
    idents = ["ctx", "slot", "n_blocks", "offset", "len", "rc", "out", "in_buf", "crc", "i", "k", "state", "hdr", "next_event"]
    types = ["uint32_t", "uint64_t", "const uint8_t*", "int", "size_t", "bool"]
    out, depth = bytearray(), 0
    while len(out) < n:
        ind = b"    " * depth
        k = r.randrange(10)
        if k < 3:
            out += ind + ("%s %s = %s + %d;\n" % (r.choice(types), r.choice(idents), r.choice(idents), r.randrange(64))).encode()
        elif k < 5:
            out += ind + ("if (%s %s %s) {\n" % (r.choice(idents), r.choice(["<", ">=", "==", "!="]), r.choice(idents))).encode()
            depth += 1
        elif k < 6:
            out += ind + ("for (%s %s = 0; %s < %s; ++%s) {\n" % ((r.choice(types),) + (r.choice(idents),) * 2 + (r.choice(idents),) + (r.choice(idents),))).encode()
            depth += 1
        elif k < 8 and depth:
            depth -= 1
            out += b"    " * depth + b"}\n"
        elif k < 9:
            out += ind + ("%s = %s(%s, %s);  // %s\n" % (r.choice(idents), r.choice(["fill", "launch", "reserve", "emit"]), r.choice(idents), r.choice(idents),
                                                        r.choice(X.WORDS))).encode()
        else:
            out += ind + ("return %s;\n" % r.choice(idents)).encode()
        depth = min(depth, 6)
    return bytes(out[:n])


def fibonacci(nsym=26, seed=14):
    """Byte value i occurs fib(i) times, shuffled: a Huffman code without a limit would be nsym - 1 bits deep."""
    r = random.Random(seed)
    a, b, vals = 1, 1, []
    for i in range(nsym):
        vals += [i] * a
        a, b = b, a + b
    r.shuffle(vals)
    return bytes(vals)


@functools.lru_cache(maxsize=None)
def cases():
    P = PIECE
    c = []
    for n in (0, 1, 2, 3, 4, 5, P - 1, P, P + 1, 2 * P, 2 * P + 1):
        c.append(("text_%d" % n, X.text(n, seed=20 + n % 7) if n else b""))
    c.append(("one_byte_3", b"zzz"))                       # one distinct byte: 3 symbols, two tables, one selector
    c.append(("one_byte_piece", b"\x00" * P))             # periodic after RLE1 (four zeros and a count of 255, over and over)
    c.append(("one_byte_1000", b"z" * 1000))
    c.append(("ab_x_1000", b"ab" * 1000))                  # periodic: 1000 ties at origPtr
    c.append(("abc_x_700", b"abc" * 700))
    c.append(("ab_piece_and_a_half", b"ab" * (P * 3 // 4)))
    c.append(("runs_of_four_piece", runs_of_four(P)))     # RLE1 gives P * 5 / 4 = 99 840: the cap at its edge
    c.append(("runs_of_four_two_pieces", runs_of_four(2 * P)))
    for n in (255, 258, 259, 260, 263, 518):
        c.append(("run_%d" % n, b"x" + b"r" * n + b"y"))
        c.append(("run_%d_alone" % n, b"r" * n))
    for k in range(0, 6):  # a run across a piece boundary at every split of its first five bytes
        c.append(("run_across_%d" % k, X.text(P - k, seed=31) + b"\x07" * 300 + X.text(100, seed=32)))
    c.append(("all_256_values", all_bytes(20000)))
    c.append(("one_map_row", one_row(5000)))
    c.extend(sorted_runs())
    c.append(("random32k_repeated", (X.rnd(32768, seed=41) * 3)[:P]))  # doubling runs to its last rounds
    c.append(("text_300k", X.text(300000, seed=42)))
    c.append(("sources_like_200k", sources_like(200000)))
    c.append(("sprinkled", X.sprinkled(300, 40, seed=43, times=3000)))  # random bytes with short copies
    c.append(("random_100k", X.rnd(100000, seed=44)))
    c.append(("six_pieces", X.text(5 * P + 1234, seed=45)))
    return c


@functools.lru_cache(maxsize=None)
def big_cases():
    """(name, data, level): one block only above level 1."""
    return [
        ("zero_run_2^16-1", b"ab" * (1 << 16), 9),
        ("zero_run_2^16", b"ab" * ((1 << 16) + 1), 9),
        ("zero_run_2^16+1", b"ab" * ((1 << 16) + 2), 9),
        ("fibonacci", fibonacci(), 9),
    ]


NMTF_LIMITS = (199, 200, 599, 600, 1199, 1200, 2399, 2400)


def nmtf_cases(nmtf_of):
    """Inputs whose one block has exactly the MTF symbol counts at which the table count changes, found with the host model
    (nmtf_of(data) -> nMTF): random bytes, a symbol a byte but for the zero runs."""
    out = []
    for target in NMTF_LIMITS:
        for n in range(max(1, target - 120), target + 2):
            d = X.rnd(n, seed=1000 + target)
            if nmtf_of(d) == target:
                out.append(("nmtf_%d" % target, d))
                break
        else:
            raise AssertionError("no input with nMTF %d" % target)
    return out
