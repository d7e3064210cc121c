// sha256_core.h -- SHA-256 (FIPS 180-4 sec. 6.2, padding sec. 5.1.1), shared by sha256_ranges_kernel
// (sha256_kernels.hip), the library's host side (xz_host.cpp: the .xz container's Check id 10) and a host harness in
// tests/, the way crc_core.h and bzip2_core.h serve both sides.
//
// gfx950 mapping, as in sha512_core.h whose 32-bit building blocks it uses: a rotate is one v_alignbit_b32 of a word with
// itself, a three-way xor, Ch and Maj are one v_bitop3_b32 each, K arrives through scalar loads (the kernel keeps it in
// the constant address space).  64 rounds of 32-bit work a 64-byte block.
//
// A message of len bytes takes sha256_blocks(len) blocks.  The whole ones are read as sixteen big-endian words; the last
// one or two are formed by sha256_tail_block from a byte fetcher: the message's rest, 0x80, zeros, the bit length.
//
// The kernel reads a range that begins at any byte address with aligned 16-byte loads: sha256_range_words says how many
// aligned words overlap the range (no other is read), sha256_lane_words turns the twenty dwords a block touches into its
// sixteen message words by a funnel shift, and sha256_lane_serial is a lane's whole course, one range from the first
// word to the digest, over a fetcher of aligned words: the kernel's lane runs these steps with the wave's loads in the
// fetcher's place, the harness runs them as they stand and counts the fetches.
#pragma once
#include <stdint.h>

#include "sha512_core.h"

namespace snaphash {

#define SNAPHASH_K256_LIST                                                                                                      \
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, \
    0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, \
    0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, \
    0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, \
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, \
    0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, \
    0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u

static constexpr uint32_t K256[64] = {SNAPHASH_K256_LIST};
static constexpr uint32_t IV256[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};

constexpr uint32_t kSha256Block = 64;  // bytes of a block
constexpr uint32_t kSha256Digest = 32; // bytes of a digest
// what sha256_ranges_kernel moves at a time (here, where the host tests see them): a block a range and step -- the
// prefetch runs one step ahead -- in 16-byte loads, into a tile row of the carry word and the step's four
constexpr uint32_t kSha256Load = 16, kSha256Step = 64, kSha256TileRow = 80;

template <int N> // 0 < N < 32: one v_alignbit_b32 (the host compiler knows the shift pair as its rotate)
SH_HD uint32_t rotr32(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return alignbit(x, x, N);
#else
    return x >> N | x << (32 - N);
#endif
}
SH_HD uint32_t xor3_32(uint32_t a, uint32_t b, uint32_t c) { return bitop3<0x96>(a, b, c); }
SH_HD uint32_t big_sigma0_256(uint32_t a) { return xor3_32(rotr32<2>(a), rotr32<13>(a), rotr32<22>(a)); }
SH_HD uint32_t big_sigma1_256(uint32_t e) { return xor3_32(rotr32<6>(e), rotr32<11>(e), rotr32<25>(e)); }
SH_HD uint32_t small_sigma0_256(uint32_t x) { return xor3_32(rotr32<7>(x), rotr32<18>(x), x >> 3); }
SH_HD uint32_t small_sigma1_256(uint32_t x) { return xor3_32(rotr32<17>(x), rotr32<19>(x), x >> 10); }

#define SNAPHASH_ROUND256(a, b, c, d, e, f, g, h, kw)                                \
    do {                                                                             \
        const uint32_t t1_ = h + big_sigma1_256(e) + bitop3<0xCA>(e, f, g) + (kw);   \
        const uint32_t t2_ = big_sigma0_256(a) + bitop3<0xE8>(a, b, c);              \
        d += t1_;                                                                    \
        h = t1_ + t2_;                                                               \
    } while (0)

// One 64-byte block.  w[16]: the big-endian message words, clobbered (the rolling schedule window).  The chaining value
// moves only where `live` is true: a lane whose range has ended rides along.  kt: the 64 round constants.
SH_HD void sha256_compress(uint32_t H[8], uint32_t w[16], bool live, const uint32_t* kt)
{
    uint32_t a = H[0], b = H[1], c = H[2], d = H[3], e = H[4], f = H[5], g = H[6], h = H[7];
    // four groups of 16 rounds, the group's body unrolled and the group loop not (sha512_core.h compress_block)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int g16 = 0; g16 < 64; g16 += 16) {
        if (g16) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int t = 0; t < 16; ++t) w[t] += small_sigma1_256(w[(t + 14) & 15]) + w[(t + 9) & 15] + small_sigma0_256(w[(t + 1) & 15]);
        }
        const uint32_t* k = kt + g16;
        SNAPHASH_ROUND256(a, b, c, d, e, f, g, h, k[0] + w[0]);
        SNAPHASH_ROUND256(h, a, b, c, d, e, f, g, k[1] + w[1]);
        SNAPHASH_ROUND256(g, h, a, b, c, d, e, f, k[2] + w[2]);
        SNAPHASH_ROUND256(f, g, h, a, b, c, d, e, k[3] + w[3]);
        SNAPHASH_ROUND256(e, f, g, h, a, b, c, d, k[4] + w[4]);
        SNAPHASH_ROUND256(d, e, f, g, h, a, b, c, k[5] + w[5]);
        SNAPHASH_ROUND256(c, d, e, f, g, h, a, b, k[6] + w[6]);
        SNAPHASH_ROUND256(b, c, d, e, f, g, h, a, k[7] + w[7]);
        SNAPHASH_ROUND256(a, b, c, d, e, f, g, h, k[8] + w[8]);
        SNAPHASH_ROUND256(h, a, b, c, d, e, f, g, k[9] + w[9]);
        SNAPHASH_ROUND256(g, h, a, b, c, d, e, f, k[10] + w[10]);
        SNAPHASH_ROUND256(f, g, h, a, b, c, d, e, k[11] + w[11]);
        SNAPHASH_ROUND256(e, f, g, h, a, b, c, d, k[12] + w[12]);
        SNAPHASH_ROUND256(d, e, f, g, h, a, b, c, k[13] + w[13]);
        SNAPHASH_ROUND256(c, d, e, f, g, h, a, b, k[14] + w[14]);
        SNAPHASH_ROUND256(b, c, d, e, f, g, h, a, k[15] + w[15]);
    }
    if (live) {
        H[0] += a; H[1] += b; H[2] += c; H[3] += d;
        H[4] += e; H[5] += f; H[6] += g; H[7] += h;
    }
}

// the blocks the compression function runs for a message of len bytes: its bytes, 0x80 and the 8-byte bit length
SH_HD uint64_t sha256_blocks(uint64_t len) { return (len + 9 + 63) / 64; }

// A block behind the message's last whole one, into w.  pad_index 0: the message's last rem (< 64) bytes -- byte(j) for
// j < rem, asked for no other j --, 0x80, zeros, and the bit length if it fits (rem < 56); pad_index 1 (only when
// rem >= 56): zeros and the bit length.
template <class BYTE>
SH_HD void sha256_tail_block(uint32_t w[16], uint32_t pad_index, uint32_t rem, uint64_t len, BYTE byte)
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < 16; ++k) {
        uint32_t v = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t j = 4 * k + i;
            uint32_t c = 0;
            if (pad_index == 0 && j < rem) c = byte(j);
            else if (pad_index == 0 && j == rem) c = 0x80;
            v = v << 8 | c;
        }
        w[k] = v;
    }
    if (pad_index == 1 || rem < 56) {
        w[14] = (uint32_t)(len >> 29);
        w[15] = (uint32_t)(len << 3);
    }
}

// the digest's bytes: the eight words, big-endian
SH_HD void sha256_store_digest(uint8_t* out, const uint32_t H[8])
{
    for (int k = 0; k < 8; ++k) {
        out[4 * k] = (uint8_t)(H[k] >> 24);
        out[4 * k + 1] = (uint8_t)(H[k] >> 16);
        out[4 * k + 2] = (uint8_t)(H[k] >> 8);
        out[4 * k + 3] = (uint8_t)H[k];
    }
}

// The message p[0 .. n) on this thread: what the host side computes.  (p may be null when n is 0.)
inline void sha256_host(const uint8_t* p, uint64_t n, uint8_t out[32])
{
    uint32_t H[8], w[16];
    for (int k = 0; k < 8; ++k) H[k] = IV256[k];
    const uint64_t nfull = n / 64, nblk = sha256_blocks(n);
    const uint32_t rem = (uint32_t)(n % 64);
    for (uint64_t b = 0; b < nblk; ++b) {
        const uint8_t* q = p + b * 64;
        if (b < nfull)
            for (int k = 0; k < 16; ++k) w[k] = (uint32_t)q[4 * k] << 24 | (uint32_t)q[4 * k + 1] << 16 | (uint32_t)q[4 * k + 2] << 8 | q[4 * k + 3];
        else
            sha256_tail_block(w, (uint32_t)(b - nfull), rem, n, [&](uint32_t j) { return (uint32_t)p[nfull * 64 + j]; });
        sha256_compress(H, w, true, K256);
    }
    sha256_store_digest(out, H);
}

// ---- a range at any byte address, read in aligned 16-byte words ------------------------------------------------------------

// A range begins sh = address & 15 bytes into aligned word 0.  The aligned words that overlap it: 0 .. sha256_range_words.
SH_HD uint64_t sha256_range_words(uint32_t sh, uint64_t len) { return len ? (sh + len + 15) / 16 : 0; }

// Block b of the range lies in the aligned words 4b .. 4b + 4: d[0 .. 20) holds them as the dwords they are in memory
// (little-endian; a word that was not read holds anything).  Its sixteen message words: selects by the dwords of sh,
// then a funnel shift (v_alignbit_b32) by its bytes.  Every index is a constant: the words stay in registers.
SH_HD uint32_t sha256_pick(bool c, uint32_t a, uint32_t b) { return c ? a : b; }
SH_HD void sha256_lane_words(uint32_t w[16], const uint32_t d[20], uint32_t sh)
{
    // (two steps, by two dwords and by one, each a select between values: `c ? d[i] : d[j]` is a select between places,
    // which becomes a variable index and sends the array to scratch)
    const bool by2 = (sh & 8) != 0, by1 = (sh & 4) != 0;
    const uint32_t s = (sh & 3) * 8;
    uint32_t u[18], t[17];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 18; ++k) u[k] = sha256_pick(by2, d[k + 2], d[k]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 17; ++k) t[k] = sha256_pick(by1, u[k + 1], u[k]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 16; ++k) w[k] = __builtin_bswap32(alignbit(t[k + 1], t[k], s));
}

// A lane's course over one range of len bytes that begins sh bytes into aligned word 0.  word(j, q) puts the aligned word
// j into q[0 .. 4) and is asked for j < sha256_range_words(sh, len) alone, each j once: word 0 first (the carry), then four
// more a block, which leave the last of them as the next block's carry.  The tail's bytes are read where the block's
// twenty dwords lie (the kernel: its row of the LDS tile).
template <class WORD>
inline void sha256_lane_serial(uint32_t sh, uint64_t len, uint8_t out[32], WORD word)
{
    uint32_t H[8], w[16], d[20] = {0};
    for (int k = 0; k < 8; ++k) H[k] = IV256[k];
    const uint64_t nw = sha256_range_words(sh, len), nfull = len / 64, nblk = sha256_blocks(len);
    const uint32_t rem = (uint32_t)(len % 64);
    if (nw) word(0, d);
    for (uint64_t b = 0; b < nblk; ++b) {
        for (uint32_t i = 1; i <= 4; ++i) {
            const uint64_t j = 4 * b + i;
            if (j < nw) word(j, d + 4 * i);
            else d[4 * i] = d[4 * i + 1] = d[4 * i + 2] = d[4 * i + 3] = 0;
        }
        if (b < nfull) {
            sha256_lane_words(w, d, sh);
        } else {
            const uint8_t* bytes = (const uint8_t*)d;
            sha256_tail_block(w, (uint32_t)(b - nfull), rem, len, [&](uint32_t j) { return (uint32_t)bytes[sh + j]; });
        }
        sha256_compress(H, w, true, K256);
        for (int k = 0; k < 4; ++k) d[k] = d[16 + k];
    }
    sha256_store_digest(out, H);
}

} // namespace snaphash
