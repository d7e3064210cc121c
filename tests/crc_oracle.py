"""The CRC oracles of the CRC tests (never the code under test): zlib.crc32 for gzip's flavour, and for bzip2's a table
CRC (MSB first, polynomial 0x04C11DB7, init and final xor ~0) that check_bz_oracle() holds against libbz2 itself -- a
one-block stream stores its block CRC at bytes 10..13."""
import bz2
import zlib

GZIP, BZIP2 = 0, 1

_T = []
for _b in range(256):
    _c = _b << 24
    for _ in range(8):
        _c = ((_c << 1) ^ 0x04C11DB7 if _c & 0x80000000 else _c << 1) & 0xFFFFFFFF
    _T.append(_c)


def bz_crc(data, crc=0):
    """bzip2's CRC-32 of data, continued from a finished crc (0 to start), as zlib.crc32 is."""
    c = crc ^ 0xFFFFFFFF
    for b in bytes(data):
        c = ((c << 8) & 0xFFFFFFFF) ^ _T[(c >> 24) ^ b]
    return c ^ 0xFFFFFFFF


def bz_crc_np(data):
    """The same over a large buffer, in numpy: the register is linear, so the CRC of the whole is folded from 256 columns
    advanced together (column j holds the bytes at j, j + cols, ...), each then run on by the zero bytes behind it."""
    import numpy as np
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    if len(a) < 4096:
        return bz_crc(a.tobytes())
    T = np.array(_T, dtype=np.uint32)
    # cut into 256 contiguous pieces of equal length (the rest by the scalar loop), a register each, stepped together
    m = len(a) // 256
    rows = a[:m * 256].reshape(256, m)
    reg = np.zeros(256, dtype=np.uint32)
    reg[0] = 0xFFFFFFFF
    for j in range(m):
        reg = (reg << np.uint32(8)) ^ T[(reg >> np.uint32(24)) ^ rows[:, j]]
    # fold: piece i is followed by (255 - i) * m bytes; run its register over that many zero bytes by repeated squaring
    # of the "m zero bytes" map, applied to all registers still in front
    acc = 0
    for i in range(256):
        acc = _zeros(acc, m) ^ int(reg[i])
    c = acc
    for b in a[m * 256:].tobytes():
        c = ((c << 8) & 0xFFFFFFFF) ^ _T[(c >> 24) ^ b]
    return c ^ 0xFFFFFFFF


def _mul(a, b):
    p = 0
    for i in range(32):
        if a >> i & 1:
            p ^= b
        b = ((b << 1) ^ 0x04C11DB7 if b & 0x80000000 else b << 1) & 0xFFFFFFFF
    return p


_POW = {}


def _zeros(reg, n):
    """The register after n zero bytes: reg * x^(8n) mod P (textbook, independent of crc_core.h; checked against the byte
    loop by check_bz_oracle)."""
    if n not in _POW:
        r, base, k = 1, 0x100, n
        while k:
            if k & 1:
                r = _mul(r, base)
            base = _mul(base, base)
            k >>= 1
        _POW[n] = r
    return _mul(reg, _POW[n])


def check_bz_oracle():
    import random
    rnd = random.Random(5)
    for n in (0, 1, 5, 1000, 70001):
        buf = bytes(rnd.getrandbits(8) for _ in range(n))
        z = bz2.compress(buf, 1)
        if n:
            assert z[4:10] == bytes.fromhex("314159265359")
            assert int.from_bytes(z[10:14], "big") == bz_crc(buf), n
        assert bz_crc_np(buf) == bz_crc(buf), n


def crc(kind, data):
    return zlib.crc32(data) & 0xFFFFFFFF if kind == GZIP else bz_crc_np(data)
