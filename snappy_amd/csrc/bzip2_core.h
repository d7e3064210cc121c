// bzip2_core.h -- the bzip2 decoder of the install side's second data-member format (data.tar.bz2), shared by the GPU
// kernels (bzip2_kernels.hip), the library's host decoder (bzip2_host.cpp) and a host harness in tests/, the way
// inflate_core.h serves the gzip side.
//
// A bzip2 stream is "BZh" + a level digit, then blocks, each starting with the 48-bit magic 0x314159265359 at any bit
// offset (bits go MSB first), then the end-of-stream magic 0x177245385090, the combined CRC and padding to a byte.  A
// block needs nothing from any other block, so the routines here take one block at a time, in stages that the kernels
// run separately:
//   bz_block_symbols  the header (CRC, origPtr, used-byte map, Huffman tables, selectors) and the Huffman + RUNA/RUNB +
//                     MTF decode into the block's BWT bytes (and their 256 counts)
//   bz_ibwt           the inverse Burrows-Wheeler transform (the T vector by a counting sort, then the walk from origPtr)
//   bz_samples ..     the same walk split at sampled positions, as the kernels run it in parallel (the sample geometry,
//   bz_sample_write   one piece's walk, the link of the pieces through origPtr, one piece's output)
//   bz_rle1_step      one byte of the undo of the initial run-length stage (four equal bytes, then a count 0-255)
//   bz_crc_*          bzip2's CRC-32 (MSB first, not reflected), over a block's output after RLE1 is undone
//
// Every path is bounded: input past the end reads as zeros and ends the run as kBzTruncated, output past `cap` ends it
// as kBzOverflow, anything malformed (or what Go's compress/bzip2 refuses: the randomised bit, origPtr >= the symbol
// count) as kBzBad -- a false block start or a corrupt stream never reads or writes out of bounds.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BZ_HD __host__ __device__ inline
#else
#define BZ_HD inline
#endif

namespace snaphash {

constexpr uint64_t kBzBlockMagic = 0x314159265359ull;
constexpr uint64_t kBzEosMagic = 0x177245385090ull;
constexpr uint32_t kBzMaxBlock = 900000;     // symbols of a level-9 block (level x 100 000)
constexpr uint32_t kBzMaxSelectors = 18002;  // libbz2's BZ_MAX_SELECTORS: a 900k block needs 18 000; more are read, not kept
constexpr uint32_t kBzFastBits = 10;         // first-level lookup of a Huffman code (longer codes, up to 20 bits: canonical walk)
constexpr uint32_t kBzMaxRun = 1u << 21;     // RUNA/RUNB weight past which a run is refused (libbz2: 2 Mi)

enum : int32_t {
    kBzOk = 0,        // the block decoded to its end-of-block symbol
    kBzTruncated = 2, // the input ended first
    kBzOverflow = 3,  // more symbols than cap
    kBzBad = 4,       // not a valid block (or one Go refuses)
};

// What the symbol stage of one block leaves: where it ended, its symbol count, origPtr, the stored block CRC.
struct BzBlockRes {
    uint64_t end_bit = 0;
    uint32_t n = 0;
    uint32_t orig_ptr = 0;
    uint32_t crc = 0;
    int32_t status = kBzBad;
};

// Huffman tables and selectors of one block (about 35 KiB: it fits a workgroup's LDS).
struct BzTables {
    uint8_t sel[kBzMaxSelectors];           // the selectors, MTF undone
    uint16_t fast[6][1u << kBzFastBits];    // (length << 9) | symbol for codes of up to kBzFastBits bits; 0: a longer code
    uint32_t first[6][21];                  // canonical code of the first symbol of each length
    uint16_t count[6][21];                  // symbols of each length
    uint16_t offs[6][21];                   // symbols of shorter lengths
    uint16_t sorted[6][258];                // symbols in code order
    uint8_t unseq[256];                     // MTF alphabet -> byte value (the used-byte map)
    uint8_t mtf[256];
};

struct BzBits {
    const uint8_t* in;
    uint64_t n;   // input bytes
    uint64_t pos; // next byte to load (may pass n: the bytes past the end read as zeros)
    uint64_t buf; // bits left-aligned: the next bit is bit 63
    uint32_t cnt; // bits in buf
};

BZ_HD void bb_fill(BzBits& b)
{
    while (b.cnt <= 56) {
        const uint64_t v = b.pos < b.n ? b.in[b.pos] : 0;
        b.buf |= v << (56 - b.cnt);
        ++b.pos;
        b.cnt += 8;
    }
}
BZ_HD uint64_t bb_consumed(const BzBits& b) { return b.pos * 8 - b.cnt; }
BZ_HD bool bb_over(const BzBits& b) { return b.pos > b.n && bb_consumed(b) > b.n * 8; }
BZ_HD uint32_t bb_peek(const BzBits& b, uint32_t k) { return (uint32_t)(b.buf >> (64 - k)); } // 1 <= k <= 32
BZ_HD uint32_t bb_take(BzBits& b, uint32_t k) // 1 <= k <= 32, after bb_fill left enough bits
{
    const uint32_t v = bb_peek(b, k);
    b.buf <<= k;
    b.cnt -= k;
    return v;
}
BZ_HD void bb_start(BzBits& b, const uint8_t* in, uint64_t n, uint64_t bit)
{
    b.in = in;
    b.n = n;
    b.pos = bit >> 3;
    b.buf = 0;
    b.cnt = 0;
    bb_fill(b);
    if (bit & 7) bb_take(b, (uint32_t)(bit & 7));
}

// The 48 bits at `bit` of in[0..n) (zeros past the end).
BZ_HD uint64_t bz_bits48(const uint8_t* in, uint64_t n, uint64_t bit)
{
    BzBits b;
    bb_start(b, in, n, bit);
    const uint64_t hi = bb_take(b, 24);
    return hi << 24 | bb_take(b, 24);
}

// bzip2's CRC-32: polynomial 0x04C11DB7, MSB first; a block's CRC is ~bz_crc_update(t, ~0u, bytes).
BZ_HD void bz_crc_table(uint32_t* t)
{
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i << 24;
        for (int k = 0; k < 8; ++k) c = (c & 0x80000000u) ? (c << 1) ^ 0x04C11DB7u : c << 1;
        t[i] = c;
    }
}
BZ_HD uint32_t bz_crc_update(const uint32_t* t, uint32_t crc, const uint8_t* p, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i) crc = (crc << 8) ^ t[(crc >> 24) ^ p[i]];
    return crc;
}
BZ_HD uint32_t bz_crc_combine(uint32_t combined, uint32_t block_crc) { return ((combined << 1) | (combined >> 31)) ^ block_crc; }

// One table from its code lengths (1..20).  false for an over-subscribed code (no encoder writes one); an incomplete
// code is accepted, and its unused codes are refused when they occur.
BZ_HD bool bz_build(BzTables& t, uint32_t g, const uint8_t* len, uint32_t alpha)
{
    for (uint32_t l = 0; l < 21; ++l) t.count[g][l] = 0;
    for (uint32_t s = 0; s < alpha; ++s) t.count[g][len[s]]++;
    uint32_t code = 0, off = 0;
    for (uint32_t l = 1; l < 21; ++l) {
        t.first[g][l] = code;
        t.offs[g][l] = (uint16_t)off;
        if (code + t.count[g][l] > (1u << l)) return false;
        code = (code + t.count[g][l]) << 1;
        off += t.count[g][l];
    }
    uint16_t next[21];
    for (uint32_t l = 1; l < 21; ++l) next[l] = t.offs[g][l];
    for (uint32_t s = 0; s < alpha; ++s) t.sorted[g][next[len[s]]++] = (uint16_t)s;
    for (uint32_t i = 0; i < (1u << kBzFastBits); ++i) t.fast[g][i] = 0;
    for (uint32_t l = 1; l <= kBzFastBits; ++l)
        for (uint32_t k = 0; k < t.count[g][l]; ++k) {
            const uint32_t c = t.first[g][l] + k, s = t.sorted[g][t.offs[g][l] + k];
            const uint32_t lo = c << (kBzFastBits - l), hi = (c + 1) << (kBzFastBits - l);
            for (uint32_t f = lo; f < hi; ++f) t.fast[g][f] = (uint16_t)(l << 9 | s);
        }
    return true;
}

// One symbol of table g; -1 for bits that are no code.  Needs 20 bits in the buffer.
BZ_HD int32_t bz_decode(BzBits& b, const BzTables& t, uint32_t g)
{
    const uint32_t e = t.fast[g][bb_peek(b, kBzFastBits)];
    if (e) {
        bb_take(b, e >> 9);
        return (int32_t)(e & 511);
    }
    for (uint32_t l = kBzFastBits + 1; l < 21; ++l) {
        const uint32_t v = bb_peek(b, l) - t.first[g][l];
        if (v < t.count[g][l]) {
            bb_take(b, l);
            return t.sorted[g][t.offs[g][l] + v];
        }
    }
    return -1;
}

// The block whose magic starts at `bit`: header and symbols into bwt[0..cap) (cap <= kBzMaxBlock), their byte counts
// into counts[256] (may be null).  The result's end_bit is the first bit after the end-of-block symbol.
BZ_HD BzBlockRes bz_block_symbols(const uint8_t* in, uint64_t n, uint64_t bit, uint8_t* bwt, uint32_t cap, uint32_t* counts, BzTables& t)
{
    BzBlockRes r;
    BzBits b;
    bb_start(b, in, n, bit);
#define BZ_END(st)                   \
    {                                \
        r.status = (st);             \
        r.end_bit = bb_consumed(b);  \
        return r;                    \
    }
    const uint64_t m = (uint64_t)bb_take(b, 24) << 24;
    if ((m | bb_take(b, 24)) != kBzBlockMagic) BZ_END(kBzBad);
    bb_fill(b);
    r.crc = bb_take(b, 32);
    if (bb_take(b, 1)) BZ_END(kBzBad); // randomised: Go refuses it ("deprecated randomized files")
    r.orig_ptr = bb_take(b, 24);
    bb_fill(b);
    const uint32_t used16 = bb_take(b, 16);
    uint32_t nin = 0;
    for (uint32_t i = 0; i < 16; ++i) {
        if (!(used16 & (0x8000u >> i))) continue;
        bb_fill(b);
        const uint32_t w = bb_take(b, 16);
        for (uint32_t j = 0; j < 16; ++j)
            if (w & (0x8000u >> j)) t.unseq[nin++] = (uint8_t)(i * 16 + j);
    }
    if (bb_over(b)) BZ_END(kBzTruncated);
    if (nin == 0) BZ_END(kBzBad);
    const uint32_t alpha = nin + 2; // RUNA, RUNB, MTF indices 1 .. nin-1, EOB
    bb_fill(b);
    const uint32_t ngroups = bb_take(b, 3), nsel = bb_take(b, 15);
    if (ngroups < 2 || ngroups > 6 || nsel == 0) BZ_END(kBzBad);
    uint8_t gm[6] = {0, 1, 2, 3, 4, 5}; // the selectors' MTF list
    for (uint32_t i = 0; i < nsel; ++i) {
        uint32_t j = 0;
        for (;;) {
            bb_fill(b);
            if (bb_over(b)) BZ_END(kBzTruncated);
            if (!bb_take(b, 1)) break;
            if (++j >= ngroups) BZ_END(kBzBad);
        }
        const uint8_t v = gm[j];
        for (; j > 0; --j) gm[j] = gm[j - 1];
        gm[0] = v;
        if (i < kBzMaxSelectors) t.sel[i] = v;
    }
    const uint32_t nsel_kept = nsel < kBzMaxSelectors ? nsel : kBzMaxSelectors;
    uint8_t len[258];
    for (uint32_t g = 0; g < ngroups; ++g) {
        bb_fill(b);
        int32_t cur = (int32_t)bb_take(b, 5);
        for (uint32_t s = 0; s < alpha; ++s) {
            for (;;) {
                if (cur < 1 || cur > 20) BZ_END(kBzBad);
                bb_fill(b);
                if (bb_over(b)) BZ_END(kBzTruncated);
                if (!bb_take(b, 1)) break;
                cur += bb_take(b, 1) ? -1 : 1;
            }
            len[s] = (uint8_t)cur;
        }
        if (!bz_build(t, g, len, alpha)) BZ_END(kBzBad);
    }
    for (uint32_t i = 0; i < 256; ++i) t.mtf[i] = (uint8_t)i;
    if (counts)
        for (uint32_t i = 0; i < 256; ++i) counts[i] = 0;
    const uint32_t eob = nin + 1;
    uint32_t o = 0, run = 0, weight = 1, group = 0, left = 0, table = 0;
    for (;;) {
        if (left == 0) {
            if (group >= nsel_kept) BZ_END(kBzBad);
            table = t.sel[group++];
            left = 50;
        }
        --left;
        bb_fill(b);
        const int32_t s = bz_decode(b, t, table);
        if (bb_over(b)) BZ_END(kBzTruncated);
        if (s < 0) BZ_END(kBzBad);
        if (s <= 1) { // RUNA / RUNB: a bijective base-2 count of the front byte
            if (weight >= kBzMaxRun) BZ_END(kBzBad);
            run += weight << s;
            weight <<= 1;
            continue;
        }
        if (run) {
            if (run > cap - o) BZ_END(kBzOverflow);
            const uint8_t v = t.unseq[t.mtf[0]];
            for (uint32_t k = 0; k < run; ++k) bwt[o + k] = v;
            if (counts) counts[v] += run;
            o += run;
            run = 0;
            weight = 1;
        }
        if ((uint32_t)s == eob) break;
        const uint32_t idx = (uint32_t)s - 1; // 1 .. nin-1
        const uint8_t v = t.mtf[idx];
        for (uint32_t k = idx; k > 0; --k) t.mtf[k] = t.mtf[k - 1];
        t.mtf[0] = v;
        if (o >= cap) BZ_END(kBzOverflow);
        const uint8_t c = t.unseq[v];
        bwt[o++] = c;
        if (counts) counts[c]++;
    }
    r.n = o;
    if (r.orig_ptr >= o) BZ_END(kBzBad); // (also the empty block: Go and libbz2 refuse both)
    BZ_END(kBzOk);
#undef BZ_END
}

// The inverse BWT of bwt[0..n) (counts: its byte histogram) into out[0..n); tt[0..n) is scratch.  origPtr < n.
// tt[j] = (i << 8) | bwt[j], where the stable counting sort moved position i to j: the walk's next position and the
// byte it emits come from one load (libbz2's layout).
BZ_HD void bz_ibwt(const uint8_t* bwt, uint32_t n, const uint32_t* counts, uint32_t orig_ptr, uint32_t* tt, uint8_t* out)
{
    uint32_t cft[256];
    uint32_t sum = 0;
    for (uint32_t c = 0; c < 256; ++c) {
        cft[c] = sum;
        sum += counts[c];
    }
    for (uint32_t j = 0; j < n; ++j) tt[j] = bwt[j];
    for (uint32_t i = 0; i < n; ++i) tt[cft[bwt[i]]++] |= i << 8;
    uint32_t p = tt[orig_ptr] >> 8;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t e = tt[p];
        out[k] = (uint8_t)e;
        p = e >> 8;
    }
}

// The same walk split at sampled positions, the way the kernels run it (bz_ibwt_kernel; tests/bzip2_host_harness.cpp
// runs these helpers serially).  The samples are the multiples of `stride` plus origPtr; tt[j] is bz_ibwt's entry with
// kBzMark set on every sampled j.  Each sample's piece runs from it to the next sample; the pieces from origPtr's
// sample around to it again are the cycle of the permutation through origPtr, L steps.  That cycle need not pass every
// position: a block that is exactly periodic after RLE1 (u^k, k >= 2; "aa", 255 * m zero bytes) gives k cycles, each
// spelling u.  bz_ibwt's n steps from origPtr go round the cycle, so out[k] = out[k % L] -- also when L does not divide
// n, as for a corrupt block whose CRC then refuses it (libbz2 and Go walk the same way).
constexpr uint32_t kBzWalkers = 2048;       // sampled positions at the multiples of stride (1024 lanes, two each)
constexpr uint32_t kBzMark = 0x80000000u;   // a sampled position (tt's spare top bit)
constexpr uint32_t kBzIdx = 0xfffffu;       // tt[j] >> 8: a position < kBzMaxBlock < 2^20
constexpr uint32_t kBzNoPiece = ~0u;        // the offset of a sample off origPtr's cycle (it writes nothing)

struct BzSamples {
    uint32_t n, op;
    uint32_t stride; // ceil(n / kBzWalkers)
    uint32_t ns;     // samples at 0, stride, 2 stride, ... < n
    uint32_t extra;  // 1 when origPtr is no multiple of stride: sample ns
    uint32_t nsamp;  // ns + extra <= kBzWalkers + 1
};

BZ_HD BzSamples bz_samples(uint32_t n, uint32_t op) // n >= 1
{
    BzSamples g;
    g.n = n;
    g.op = op;
    g.stride = (n + kBzWalkers - 1) / kBzWalkers;
    g.ns = (n + g.stride - 1) / g.stride;
    g.extra = op % g.stride ? 1u : 0u;
    g.nsamp = g.ns + g.extra;
    return g;
}
BZ_HD bool bz_is_sample(const BzSamples& g, uint32_t j) { return j % g.stride == 0 || j == g.op; }
BZ_HD uint32_t bz_sample_pos(const BzSamples& g, uint32_t s) { return s < g.ns ? s * g.stride : g.op; }
BZ_HD uint32_t bz_sample_id(const BzSamples& g, uint32_t q) { return (q == g.op && g.extra) ? g.ns : q / g.stride; } // q a sample

// Sample s's piece: its length in steps (~0u: the walk left [0, n) or ran n steps without meeting a sample), and the
// id of the sample it ends at into *next.
BZ_HD uint32_t bz_sample_walk(const BzSamples& g, const uint32_t* tt, uint32_t s, uint32_t* next)
{
    uint32_t q = bz_sample_pos(g, s), v = tt[q], len = 0;
    for (;;) {
        q = (v >> 8) & kBzIdx;
        if (q >= g.n || len >= g.n) {
            *next = 0;
            return ~0u;
        }
        v = tt[q];
        ++len;
        if (v & kBzMark) break;
    }
    *next = bz_sample_id(g, q);
    return len;
}

// Links the pieces from origPtr's sample until the walk is back at it: soff[s] is each piece's offset in the output, or
// kBzNoPiece for a sample off that cycle.  Returns the cycle's length L (1 <= L <= n), or 0 when a piece is broken or
// the links do not come back (neither happens for a T vector built by the counting sort: it is a permutation).
BZ_HD uint32_t bz_link_samples(const BzSamples& g, const uint32_t* slen, const uint32_t* snext, uint32_t* soff)
{
    for (uint32_t s = 0; s < g.nsamp; ++s) soff[s] = kBzNoPiece;
    const uint32_t s0 = bz_sample_id(g, g.op);
    uint32_t s = s0;
    uint64_t off = 0;
    do {
        if (s >= g.nsamp || slen[s] == ~0u || soff[s] != kBzNoPiece) return 0;
        soff[s] = (uint32_t)off;
        off += slen[s];
        if (off > g.n) return 0;
        s = snext[s];
    } while (s != s0);
    return (uint32_t)off;
}

// Sample s's piece written at out[0..len) (out: the output at the piece's offset).
BZ_HD void bz_sample_write(const BzSamples& g, const uint32_t* tt, uint32_t s, uint32_t len, uint8_t* out)
{
    uint32_t q = bz_sample_pos(g, s), v = tt[q];
    for (uint32_t k = 0; k < len; ++k) {
        q = (v >> 8) & kBzIdx;
        v = tt[q];
        out[k] = (uint8_t)v;
    }
}

// The RLE1 undo's state between two bytes: run = 0 (fresh: nothing to compare with), 1..3 equal bytes `last` so far,
// or 4 (the next byte is a count of further copies of `last`).
struct BzRle1 {
    uint32_t run = 0;
    uint32_t last = 0;
};

// One byte of the RLE1 stream: returns how many bytes it decodes to (the copies are of st.last after the call when the
// byte was a count, otherwise the byte itself).
BZ_HD uint32_t bz_rle1_step(BzRle1& st, uint8_t v, bool& is_count)
{
    if (st.run == 4) {
        st.run = 0;
        is_count = true;
        return v;
    }
    is_count = false;
    if (st.run && v == st.last) {
        ++st.run;
    } else {
        st.run = 1;
        st.last = v;
    }
    return 1;
}

// RLE1 undo of in[0..n) from state st into out[0..cap); returns the bytes written, or ~0ull past cap (out may be null:
// the length alone, no cap).
BZ_HD uint64_t bz_rle1(BzRle1& st, const uint8_t* in, uint64_t n, uint8_t* out, uint64_t cap)
{
    uint64_t o = 0;
    for (uint64_t i = 0; i < n; ++i) {
        bool cnt = false;
        const uint32_t k = bz_rle1_step(st, in[i], cnt);
        if (out) {
            if (k > cap - o) return ~0ull;
            const uint8_t v = cnt ? (uint8_t)st.last : in[i];
            for (uint32_t q = 0; q < k; ++q) out[o + q] = v;
        }
        o += k;
    }
    return o;
}

} // namespace snaphash
