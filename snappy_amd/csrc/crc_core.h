// crc_core.h -- the two CRC-32s the install side checks, as polynomial arithmetic that can be cut and folded: shared by
// the GPU kernels (crc_kernels.hip), the host code (snap.inc) and a host harness in tests/, the way bzip2_core.h and
// inflate_core.h serve the decoders.
//
//   kCrcGzip   gzip's / zlib's: bits reflected (LSB first), polynomial 0xEDB88320, init and final xor ~0
//   kCrcBzip2  bzip2's: MSB first, polynomial 0x04C11DB7, init and final xor ~0
//
// Both are the remainder of M(x) * x^32 modulo P, with ~0 xor'ed over the first four bytes and over the result.  The
// register is linear in the message, so everything here works on the RAW remainder (init 0, no final xor):
//   raw(A || B) = raw(A) * x^(8 |B|)  xor  raw(B)                    (crc_combine does the same on finished CRCs:
//                                                                     the inits and final xors cancel)
//   crc(M)      = raw(M)  xor  ~0 * x^(8 |M|)  xor  ~0               (crc_finish)
// and raw() of a message does not change when zero bytes are put in FRONT of it.  That is how the kernel cuts a range:
// tiles and lane slices are laid out from the range's END, every slice of a tile and every tile of a range has the same
// (virtual) length, and each partial result is shifted to its place by a constant that depends on its index alone.
//
// A product modulo P is a shift-and-xor loop of 32 steps (gfx950 has no carry-less multiply); x^(8 n) is the product of
// the constants x^(8 * 2^j) for the set bits j of n (crc_pow_table holds the 64 of them), so n may be anything a
// uint64_t holds, 0 included.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CRC_HD __host__ __device__ inline
#else
#define CRC_HD inline
#endif

namespace snaphash {

enum : int { kCrcGzip = 0, kCrcBzip2 = 1 };

constexpr uint32_t kCrcTileLog = 16;                 // a workgroup's tile: 64 KiB
constexpr uint32_t kCrcSliceLog = 8;                 // a lane's slice of it: 256 bytes
constexpr uint32_t kCrcTile = 1u << kCrcTileLog;
constexpr uint32_t kCrcSlice = 1u << kCrcSliceLog;
constexpr uint32_t kCrcLanes = kCrcTile / kCrcSlice; // 256 lanes a workgroup

template <int KIND> struct CrcPoly;
template <> struct CrcPoly<kCrcGzip> {
    static constexpr uint32_t poly = 0xEDB88320u;
    static constexpr uint32_t one = 0x80000000u; // x^0 (bit 31 is the coefficient of x^0)
    static constexpr uint32_t x8 = 0x00800000u;  // x^8
};
template <> struct CrcPoly<kCrcBzip2> {
    static constexpr uint32_t poly = 0x04C11DB7u;
    static constexpr uint32_t one = 1u;
    static constexpr uint32_t x8 = 0x100u;
};

// a * b mod P
template <int KIND> CRC_HD uint32_t crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    if (KIND == kCrcGzip) {
        for (int i = 31; i >= 0; --i) {
            p ^= (a >> i & 1) ? b : 0;
            b = (b >> 1) ^ ((b & 1) ? CrcPoly<KIND>::poly : 0);
        }
    } else {
        for (int i = 0; i < 32; ++i) {
            p ^= (a >> i & 1) ? b : 0;
            b = (b << 1) ^ ((b >> 31) ? CrcPoly<KIND>::poly : 0);
        }
    }
    return p;
}

// pw[j] = x^(8 * 2^j) mod P, j = 0 .. 63
struct CrcPowTable {
    uint32_t pw[64];
};
template <int KIND> CRC_HD void crc_pow_table(CrcPowTable& t)
{
    uint32_t v = CrcPoly<KIND>::x8;
    for (int j = 0; j < 64; ++j) {
        t.pw[j] = v;
        v = crc_mul<KIND>(v, v);
    }
}
// x^(8 * n * 2^shift) mod P (shift + the bits of n must stay below 64)
template <int KIND> CRC_HD uint32_t crc_xpow8(const CrcPowTable& t, uint64_t n, uint32_t shift = 0)
{
    uint32_t r = CrcPoly<KIND>::one;
    for (uint32_t j = shift; n; ++j, n >>= 1)
        if (n & 1) r = crc_mul<KIND>(r, t.pw[j & 63]);
    return r;
}

// the CRC of A || B from the CRCs of A and B and the length of B (zlib's crc32_combine, for either flavour)
template <int KIND> CRC_HD uint32_t crc_combine(const CrcPowTable& t, uint32_t crc_a, uint32_t crc_b, uint64_t len_b)
{
    return crc_mul<KIND>(crc_a, crc_xpow8<KIND>(t, len_b)) ^ crc_b;
}
// the CRC of a message of len bytes from its raw remainder
template <int KIND> CRC_HD uint32_t crc_finish(const CrcPowTable& t, uint32_t raw, uint64_t len)
{
    return raw ^ crc_mul<KIND>(0xffffffffu, crc_xpow8<KIND>(t, len)) ^ 0xffffffffu;
}

// ---- the byte tables: tab[k][b] = raw remainder of byte b followed by k zero bytes (slice-by-8) --------------------------

template <int KIND> CRC_HD uint32_t crc_table0(uint32_t b)
{
    uint32_t c = KIND == kCrcGzip ? b : b << 24;
    for (int k = 0; k < 8; ++k) {
        if (KIND == kCrcGzip) c = (c >> 1) ^ ((c & 1) ? CrcPoly<KIND>::poly : 0);
        else c = (c << 1) ^ ((c >> 31) ? CrcPoly<KIND>::poly : 0);
    }
    return c;
}
// entry b of table k from table k - 1 (t0: table 0)
template <int KIND> CRC_HD uint32_t crc_table_next(const uint32_t* t0, uint32_t prev)
{
    return KIND == kCrcGzip ? (prev >> 8) ^ t0[prev & 0xff] : (prev << 8) ^ t0[prev >> 24];
}
// all eight on one thread (the host's tables; the kernel builds its own in LDS, an entry a lane)
template <int KIND> CRC_HD void crc_tables(uint32_t (*tab)[256])
{
    for (uint32_t b = 0; b < 256; ++b) tab[0][b] = crc_table0<KIND>(b);
    for (int k = 1; k < 8; ++k)
        for (uint32_t b = 0; b < 256; ++b) tab[k][b] = crc_table_next<KIND>(tab[0], tab[k - 1][b]);
}

template <int KIND> CRC_HD uint32_t crc_byte(const uint32_t (*tab)[256], uint32_t c, uint8_t b)
{
    return KIND == kCrcGzip ? (c >> 8) ^ tab[0][(c ^ b) & 0xff] : (c << 8) ^ tab[0][(c >> 24) ^ b];
}
CRC_HD uint32_t crc_bswap(uint32_t w) { return w >> 24 | (w >> 8 & 0xff00) | (w << 8 & 0xff0000) | w << 24; }
// eight bytes as two little-endian words, w0 the first four
template <int KIND> CRC_HD uint32_t crc_word8(const uint32_t (*tab)[256], uint32_t c, uint32_t w0, uint32_t w1)
{
    if (KIND == kCrcGzip) {
        c ^= w0;
        return tab[7][c & 0xff] ^ tab[6][c >> 8 & 0xff] ^ tab[5][c >> 16 & 0xff] ^ tab[4][c >> 24] ^
               tab[3][w1 & 0xff] ^ tab[2][w1 >> 8 & 0xff] ^ tab[1][w1 >> 16 & 0xff] ^ tab[0][w1 >> 24];
    }
    c ^= crc_bswap(w0);
    return tab[7][c >> 24] ^ tab[6][c >> 16 & 0xff] ^ tab[5][c >> 8 & 0xff] ^ tab[4][c & 0xff] ^
           tab[3][w1 & 0xff] ^ tab[2][w1 >> 8 & 0xff] ^ tab[1][w1 >> 16 & 0xff] ^ tab[0][w1 >> 24];
}

// The raw remainder of p[0..n) continued from c: bytes up to the first 16-byte boundary of the ADDRESS, then 16-byte
// loads, then the bytes that are left.  Nothing outside p[0..n) is read.
template <int KIND> CRC_HD uint32_t crc_raw_update(const uint32_t (*tab)[256], uint32_t c, const uint8_t* p, uint64_t n)
{
    while (n && ((uintptr_t)p & 15)) { c = crc_byte<KIND>(tab, c, *p++); --n; }
    for (; n >= 16; p += 16, n -= 16) {
#if defined(__HIP_DEVICE_COMPILE__)
        const uint4 v = *(const uint4*)p;
        const uint32_t w0 = v.x, w1 = v.y, w2 = v.z, w3 = v.w;
#else
        uint32_t w[4];
        __builtin_memcpy(w, p, 16);
        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
#endif
        c = crc_word8<KIND>(tab, c, w0, w1);
        c = crc_word8<KIND>(tab, c, w2, w3);
    }
    while (n) { c = crc_byte<KIND>(tab, c, *p++); --n; }
    return c;
}

// ---- how a range is cut (the kernel's geometry, run serially by the host harness too) ----------------------------------

CRC_HD uint64_t crc_tiles_of(uint64_t len) { return (len + kCrcTile - 1) >> kCrcTileLog; }

// Tile k of a range of len bytes, counted from the range's END, and lane `lane` of it: the lane's bytes are
// [*lo, *hi) relative to the range's start (empty: *lo == *hi).  Lane kCrcLanes - 1 ends where the tile ends; what would
// lie in front of the range's first byte is left out (virtual zeros).
CRC_HD void crc_lane_slice(uint64_t len, uint64_t k, uint32_t lane, uint64_t* lo, uint64_t* hi)
{
    const uint64_t tile_end = len - (k << kCrcTileLog);                 // > 0 for k < crc_tiles_of(len)
    const uint64_t back = (uint64_t)(kCrcLanes - 1 - lane) << kCrcSliceLog; // bytes between the slice's end and the tile's
    if (back >= tile_end) { *lo = *hi = 0; return; }
    *hi = tile_end - back;
    *lo = *hi > kCrcSlice ? *hi - kCrcSlice : 0;
}
// what lane `lane` multiplies its slice's remainder by: x^(8 * kCrcSlice * (kCrcLanes - 1 - lane))
template <int KIND> CRC_HD uint32_t crc_lane_shift(const CrcPowTable& t, uint32_t lane)
{
    return crc_xpow8<KIND>(t, kCrcLanes - 1 - lane, kCrcSliceLog);
}
// what tile k's remainder is multiplied by: x^(8 * kCrcTile * k)
template <int KIND> CRC_HD uint32_t crc_tile_shift(const CrcPowTable& t, uint64_t k)
{
    return crc_xpow8<KIND>(t, k, kCrcTileLog);
}

// ---- CRC-64/XZ (the .xz container's Check id 4) -------------------------------------------------------------------------
//
// ECMA-182 reflected: polynomial 0xC96C5795D7870F42, init and final xor ~0.  The same arithmetic as kCrcGzip on 64-bit
// remainders (bit 63 is the coefficient of x^0), the same cut of a range (crc_lane_slice, crc_tiles_of); a product is 64
// shift-and-xor steps.

constexpr uint64_t kCrc64Poly = 0xC96C5795D7870F42ull;
constexpr uint64_t kCrc64One = 1ull << 63; // x^0
constexpr uint64_t kCrc64X8 = 1ull << 55;  // x^8

CRC_HD uint64_t crc64_mul(uint64_t a, uint64_t b)
{
    uint64_t p = 0;
    for (int i = 63; i >= 0; --i) {
        p ^= (a >> i & 1) ? b : 0;
        b = (b >> 1) ^ ((b & 1) ? kCrc64Poly : 0);
    }
    return p;
}
struct Crc64PowTable {
    uint64_t pw[64]; // x^(8 * 2^j) mod P
};
CRC_HD void crc64_pow_table(Crc64PowTable& t)
{
    uint64_t v = kCrc64X8;
    for (int j = 0; j < 64; ++j) {
        t.pw[j] = v;
        v = crc64_mul(v, v);
    }
}
// x^(8 * n * 2^shift) mod P
CRC_HD uint64_t crc64_xpow8(const Crc64PowTable& t, uint64_t n, uint32_t shift = 0)
{
    uint64_t r = kCrc64One;
    for (uint32_t j = shift; n; ++j, n >>= 1)
        if (n & 1) r = crc64_mul(r, t.pw[j & 63]);
    return r;
}
CRC_HD uint64_t crc64_combine(const Crc64PowTable& t, uint64_t crc_a, uint64_t crc_b, uint64_t len_b)
{
    return crc64_mul(crc_a, crc64_xpow8(t, len_b)) ^ crc_b;
}
CRC_HD uint64_t crc64_finish(const Crc64PowTable& t, uint64_t raw, uint64_t len)
{
    return raw ^ crc64_mul(~0ull, crc64_xpow8(t, len)) ^ ~0ull;
}
CRC_HD uint64_t crc64_table0(uint32_t b)
{
    uint64_t c = b;
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1) ? kCrc64Poly : 0);
    return c;
}
CRC_HD uint64_t crc64_table_next(const uint64_t* t0, uint64_t prev) { return (prev >> 8) ^ t0[prev & 0xff]; }
CRC_HD void crc64_tables(uint64_t (*tab)[256])
{
    for (uint32_t b = 0; b < 256; ++b) tab[0][b] = crc64_table0(b);
    for (int k = 1; k < 8; ++k)
        for (uint32_t b = 0; b < 256; ++b) tab[k][b] = crc64_table_next(tab[0], tab[k - 1][b]);
}
CRC_HD uint64_t crc64_byte(const uint64_t (*tab)[256], uint64_t c, uint8_t b) { return (c >> 8) ^ tab[0][(c ^ b) & 0xff]; }
// eight bytes as one little-endian word
CRC_HD uint64_t crc64_word8(const uint64_t (*tab)[256], uint64_t c, uint64_t w)
{
    c ^= w;
    return tab[7][c & 0xff] ^ tab[6][c >> 8 & 0xff] ^ tab[5][c >> 16 & 0xff] ^ tab[4][c >> 24 & 0xff] ^ tab[3][c >> 32 & 0xff] ^
           tab[2][c >> 40 & 0xff] ^ tab[1][c >> 48 & 0xff] ^ tab[0][c >> 56];
}
// as crc_raw_update: nothing outside p[0..n) is read
CRC_HD uint64_t crc64_raw_update(const uint64_t (*tab)[256], uint64_t c, const uint8_t* p, uint64_t n)
{
    while (n && ((uintptr_t)p & 15)) { c = crc64_byte(tab, c, *p++); --n; }
    for (; n >= 16; p += 16, n -= 16) {
#if defined(__HIP_DEVICE_COMPILE__)
        const uint4 v = *(const uint4*)p;
        const uint64_t w0 = (uint64_t)v.y << 32 | v.x, w1 = (uint64_t)v.w << 32 | v.z;
#else
        uint64_t w[2];
        __builtin_memcpy(w, p, 16);
        const uint64_t w0 = w[0], w1 = w[1];
#endif
        c = crc64_word8(tab, c, w0);
        c = crc64_word8(tab, c, w1);
    }
    while (n) { c = crc64_byte(tab, c, *p++); --n; }
    return c;
}
CRC_HD uint64_t crc64_lane_shift(const Crc64PowTable& t, uint32_t lane) { return crc64_xpow8(t, kCrcLanes - 1 - lane, kCrcSliceLog); }
CRC_HD uint64_t crc64_tile_shift(const Crc64PowTable& t, uint64_t k) { return crc64_xpow8(t, k, kCrcTileLog); }

} // namespace snaphash
