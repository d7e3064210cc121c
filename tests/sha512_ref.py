"""SHA-512 (FIPS 180-4 sec. 6.4) in plain Python integers, one segment of a stream at a time: the reference for what a
kernel leaves in a state row between two segments, and for a padding whose length field no real stream reaches.  It shares
nothing with snappy_amd/csrc/sha512_core.h: the constants come from the primes' roots (sec. 4.2.3, 5.3.5), the rounds are
the standard's text.  tests/test_core_host.py holds it against hashlib.  About 0.3 ms a block: where a case is a whole
stream from the initial value, use hashlib.

A chaining value is a list of eight ints.  The byte count is 64 bits wide, as Job.total_prev and every counter of the
library are: total_prev + len(data) wraps at 2^64 (a stream of 16 EiB; the standard's own limit is 2^125 bytes)."""
import math

M64 = (1 << 64) - 1


def _primes(n):
    out, k = [], 2
    while len(out) < n:
        if all(k % p for p in out if p * p <= k):
            out.append(k)
        k += 1
    return out


def _icbrt(x):
    """floor(x ** (1/3)), exact"""
    r = 1 << -(-x.bit_length() // 3)
    while True:
        s = (2 * r + x // (r * r)) // 3
        if s >= r:
            return r
        r = s


# the first 64 bits of the fractional parts of the cube (K) and square (IV) roots: floor(root(p) * 2^64) mod 2^64
K = [_icbrt(p << 192) & M64 for p in _primes(80)]
IV = [math.isqrt(p << 128) & M64 for p in _primes(8)]


def _rotr(x, n):
    return ((x >> n) | (x << (64 - n))) & M64


def _block(H, blk):
    w = [int.from_bytes(blk[8 * t:8 * t + 8], "big") for t in range(16)]
    for t in range(16, 80):
        s0 = _rotr(w[t - 15], 1) ^ _rotr(w[t - 15], 8) ^ (w[t - 15] >> 7)
        s1 = _rotr(w[t - 2], 19) ^ _rotr(w[t - 2], 61) ^ (w[t - 2] >> 6)
        w.append((s1 + w[t - 7] + s0 + w[t - 16]) & M64)
    a, b, c, d, e, f, g, h = H
    for t in range(80):
        t1 = (h + (_rotr(e, 14) ^ _rotr(e, 18) ^ _rotr(e, 41)) + ((e & f) ^ (~e & g & M64)) + K[t] + w[t]) & M64
        t2 = ((_rotr(a, 28) ^ _rotr(a, 34) ^ _rotr(a, 39)) + ((a & b) ^ (a & c) ^ (b & c))) & M64
        a, b, c, d, e, f, g, h = (t1 + t2) & M64, a, b, c, (d + t1) & M64, e, f, g
    return [(x + y) & M64 for x, y in zip(H, (a, b, c, d, e, f, g, h))]


def segment(H, data, total_prev, final):
    """The chaining value after `data`, a segment of a stream of which total_prev bytes went before, starting from H.
    final: the padding of sec. 5.1.2 follows, for a message of total_prev + len(data) bytes; a segment that is not
    final is a whole number of blocks."""
    data = bytes(data)
    if final:
        bits = (((total_prev + len(data)) & M64) * 8).to_bytes(16, "big")
        data += b"\x80" + bytes((111 - len(data)) % 128) + bits
    assert len(data) % 128 == 0
    H = list(H)
    for o in range(0, len(data), 128):
        H = _block(H, data[o:o + 128])
    return H


def digest(H):
    return b"".join(x.to_bytes(8, "big") for x in H)
