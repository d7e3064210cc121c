// xz_enc_core.h -- the .xz writer: container assembly and the LZMA2 / LZMA encoder, shared by the GPU kernels
// (xz_enc_kernels.hip), the library's host side (xzpack.inc) and a host model in tests/, the way xz_core.h serves the
// decoders.  The container assembly is host-only, the encoder is host + device (XZ_HD).
//
// What is written: one Stream, Check CRC-64 unless the caller names another of the four this project
// reads (none, CRC-32, CRC-64, SHA-256: the container's routines take the id, CRC-64 where it is left out), a Block per
// block_size bytes of input (the last one
// shorter), every Block header stating both sizes, one LZMA2 filter with lc=3 lp=0 pb=2 and the smallest dictionary that
// holds a Block.  Inside a Block an LZMA2 chunk holds kXzEncChunk (65 536) uncompressed bytes, the one size at which both
// of LZMA2's limits hold without a second split.  Every chunk resets the coder state and sends the properties again (the
// first of a Block 0xE0 / 0x01, the later ones 0xC0 / 0x02) but keeps the dictionary: a chunk's output depends on the
// Block's bytes in front of it and on nothing another chunk's coder did, so the chunks of a Block are coded side by side
// and still match into each other's bytes.  A chunk is written as LZMA iff 6 + csize < 3 + usize and csize <= 65 536,
// as an uncompressed chunk otherwise; no end marker is written; the Block ends with the 0x00 byte.
//
// The match rules are those the head of xz_core.h lists as settled against liblzma: lengths 2..273, no match past its
// chunk's end, a distance at most the bytes since the Block's start, no rep or short rep before the first byte.
//
// The bytes are a function of (input, block_size, Check) alone.  The three steps below are pure functions of the Block:
//   xzenc_chains_host / lzma_chains_kernel   prev[p] = the nearest earlier position of the Block with the same 4-byte hash
//   xzenc_find                               the best (length, distance) at p: the chain in order, kXzEncDepth links, the
//                                            longest kept, the nearest among equals, every compare cut at the chunk's end
//   xzenc_chunk                              the parse (greedy, one step of lazy evaluation, rep0-3 first, short reps),
//                                            the symbol coder and the adaptive range encoder, one serial pass
// At level 1 (the level is then part of what the bytes are a function of) the last two are
//   xzenc_find_set                           up to kXzEncCands candidates at p: kXzEncDepthHigh links, lengths strictly rising
//   xzenc_chunk_priced                       a price-based shortest-path parse over windows, relaxed by all lanes; the same coder
#pragma once
#include <algorithm>

#include "xz_core.h"

// (inlined by force on the device: the coder's registers then never take the detour through a stack frame)
#if defined(__HIPCC__)
#define XZE_HD __host__ __device__ __forceinline__
#else
#define XZE_HD inline
#endif

namespace snaphash {

constexpr uint32_t kXzEncChunk = 65536;              // uncompressed bytes of an LZMA2 chunk
constexpr uint32_t kXzEncSlot = kXzEncChunk + 64;    // room for a chunk's coder output (what does not fit is counted, not stored)
constexpr uint64_t kXzEncBlockDefault = 1ull << 20;
constexpr uint64_t kXzEncBlockMax = 4ull << 20;      // what the install side's kernel takes (kXzGpuBlockMax)
constexpr uint32_t kXzEncHashBits = 15;
constexpr uint32_t kXzEncDepth = 8;                  // chain links examined per position
constexpr uint32_t kXzEncNone = 0xffffffffu;         // prev[]: no earlier position
constexpr uint32_t kXzEncStored = 0x80000000u;       // a chunk's result: written uncompressed (otherwise: its csize)
constexpr uint32_t kXzEncProbs = kLzmaLitBase + (0x300u << 3); // lc=3 lp=0: 7 990 probabilities, 15 980 bytes
constexpr uint32_t kXzEncProps = (2 * 5 + 0) * 9 + 3;          // pb=2 lp=0 lc=3: 0x5D

// ---- the match model ----------------------------------------------------------------------------------------------------

XZE_HD uint32_t xzenc_ld32(const uint8_t* p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
XZE_HD uint32_t xzenc_hash(uint32_t four) { return (four * 2654435761u) >> (32 - kXzEncHashBits); }

// the bytes a[0..) and b[0..) have in common, at most maxlen (a < b may overlap b: only bytes below b + maxlen are read)
XZE_HD uint32_t xzenc_common(const uint8_t* a, const uint8_t* b, uint32_t maxlen)
{
    uint32_t l = 0;
    while (l + 4 <= maxlen) {
        const uint32_t x = xzenc_ld32(a + l) ^ xzenc_ld32(b + l);
        if (x) return l + ((uint32_t)__builtin_ctz(x) >> 3);
        l += 4;
    }
    while (l < maxlen && a[l] == b[l]) ++l;
    return l;
}

// a candidate: length << 22 | distance - 1 (a Block is at most 4 MiB), 0 for none
XZE_HD uint32_t xzenc_cand_len(uint32_t c) { return c >> 22; }
XZE_HD uint32_t xzenc_cand_dist1(uint32_t c) { return c & 0x3fffffu; }

// The best match at position p of the Block blk, p in the chunk that ends at ce.  prev: the Block's chains.
XZE_HD uint32_t xzenc_find(const uint8_t* blk, const uint32_t* prev, uint32_t p, uint32_t ce)
{
    const uint32_t maxlen = ce - p < kLzmaMatchMax ? ce - p : kLzmaMatchMax;
    if (maxlen < 2) return 0;
    uint32_t best_len = 1, best_dist = 0;
    uint32_t c = prev[p];
    for (uint32_t d = 0; d < kXzEncDepth && c < p; ++d) { // (kXzEncNone fails c < p)
        const uint32_t l = xzenc_common(blk + c, blk + p, maxlen);
        if (l > best_len) {
            best_len = l;
            best_dist = p - c;
            if (l == maxlen) break;
        }
        c = prev[c];
    }
    // a short match far away costs more than its literals
    if (best_len < 2 || (best_len == 2 && best_dist > 128) || (best_len == 3 && best_dist > (1u << 14))) return 0;
    return best_len << 22 | (best_dist - 1);
}

// ---- the range encoder ---------------------------------------------------------------------------------------------------

// low is 64 bits wide: bit 32 is a carry into the bytes already shifted out, of which the last (cache) and a run of
// 0xFF bytes behind it (cache_size counts both) are held back until it is known.  Bytes past cap are counted, not stored.
struct XzRcEnc {
    uint64_t low;
    uint32_t range, cache_size, cache;
    uint8_t* out;
    uint32_t n, cap;
};

XZE_HD void xzrc_init(XzRcEnc& r, uint8_t* out, uint32_t cap)
{
    r.low = 0;
    r.range = 0xffffffffu;
    r.cache_size = 1; // the chunk's first byte: the zero the decoder asks for
    r.cache = 0;
    r.out = out;
    r.n = 0;
    r.cap = cap;
}
XZE_HD void xzrc_shift_low(XzRcEnc& r)
{
    if ((uint32_t)r.low < 0xff000000u || (r.low >> 32) != 0) {
        const uint32_t carry = (uint32_t)(r.low >> 32);
        do {
            if (r.n < r.cap) r.out[r.n] = (uint8_t)(r.cache + carry);
            ++r.n;
            r.cache = 0xff;
        } while (--r.cache_size);
        r.cache = (uint32_t)(r.low >> 24) & 0xff;
    }
    ++r.cache_size;
    r.low = (r.low & 0x00ffffffu) << 8;
}
XZE_HD void xzrc_bit(XzRcEnc& r, uint16_t* p, uint32_t bit)
{
    const uint32_t v = *p;
    const uint32_t bound = (r.range >> 11) * v;
    if (!bit) {
        r.range = bound;
        *p = (uint16_t)(v + ((2048 - v) >> 5));
    } else {
        r.low += bound;
        r.range -= bound;
        *p = (uint16_t)(v - (v >> 5));
    }
    while (r.range < (1u << 24)) {
        r.range <<= 8;
        xzrc_shift_low(r);
    }
}
XZE_HD void xzrc_direct(XzRcEnc& r, uint32_t value, uint32_t bits)
{
    for (uint32_t i = bits; i-- > 0;) {
        r.range >>= 1;
        if ((value >> i) & 1) r.low += r.range;
        while (r.range < (1u << 24)) {
            r.range <<= 8;
            xzrc_shift_low(r);
        }
    }
}
XZE_HD void xzrc_tree(XzRcEnc& r, uint16_t* p, uint32_t bits, uint32_t value)
{
    uint32_t m = 1;
    for (uint32_t i = bits; i-- > 0;) {
        const uint32_t b = (value >> i) & 1;
        xzrc_bit(r, p + m, b);
        m = (m << 1) | b;
    }
}
XZE_HD void xzrc_tree_rev(XzRcEnc& r, uint16_t* p, uint32_t bits, uint32_t value)
{
    uint32_t m = 1;
    for (uint32_t i = 0; i < bits; ++i) {
        const uint32_t b = (value >> i) & 1;
        xzrc_bit(r, p + m, b);
        m = (m << 1) | b;
    }
}
// the five-byte flush: the decoder's code is zero after its last normalisation; returns the bytes produced
XZE_HD uint32_t xzrc_finish(XzRcEnc& r)
{
    for (int i = 0; i < 5; ++i) xzrc_shift_low(r);
    return r.n;
}

// ---- the symbol coder ----------------------------------------------------------------------------------------------------

struct LzmaEnc {
    XzRcEnc rc;
    uint32_t state;
    uint32_t rep0, rep1, rep2, rep3; // distances - 1 (four names, not an array: they stay in registers on the device)
};

XZE_HD void lzmaenc_len(LzmaEnc& e, uint16_t* p, uint32_t len, uint32_t pos_state)
{
    const uint32_t l = len - 2;
    if (l < 8) {
        xzrc_bit(e.rc, p + kLenChoice, 0);
        xzrc_tree(e.rc, p + kLenLow + (pos_state << 3), 3, l);
    } else if (l < 16) {
        xzrc_bit(e.rc, p + kLenChoice, 1);
        xzrc_bit(e.rc, p + kLenChoice2, 0);
        xzrc_tree(e.rc, p + kLenMid + (pos_state << 3), 3, l - 8);
    } else {
        xzrc_bit(e.rc, p + kLenChoice, 1);
        xzrc_bit(e.rc, p + kLenChoice2, 1);
        xzrc_tree(e.rc, p + kLenHigh, 8, l - 16);
    }
}

// byte b at Block position pos (prev: the byte in front of it, 0 at the Block's start)
XZE_HD void lzmaenc_literal(LzmaEnc& e, uint16_t* probs, const uint8_t* blk, uint32_t pos, uint32_t prev)
{
    const uint32_t b = blk[pos];
    xzrc_bit(e.rc, probs + kPIsMatch + (e.state << 4) + (pos & 3), 0);
    uint16_t* p = probs + kLzmaLitBase + 0x300u * (prev >> 5);
    if (e.state < 7) {
        xzrc_tree(e.rc, p, 8, b);
    } else { // after a match: the byte the match would have continued with steers the tree while it agrees
        uint32_t mb = blk[pos - e.rep0 - 1], offs = 0x100, sym = 1;
        for (uint32_t i = 8; i-- > 0;) {
            mb <<= 1;
            const uint32_t mbit = mb & offs;
            const uint32_t bit = (b >> i) & 1;
            xzrc_bit(e.rc, p + offs + mbit + sym, bit);
            sym = (sym << 1) | bit;
            offs &= bit ? mbit : ~mbit;
        }
    }
    e.state = e.state < 4 ? 0 : e.state < 10 ? e.state - 3 : e.state - 6;
}

XZE_HD uint32_t lzmaenc_dist_slot(uint32_t d)
{
    if (d < 4) return d;
    const uint32_t nb = 31 - (uint32_t)__builtin_clz(d);
    return 2 * nb + ((d >> (nb - 1)) & 1);
}

// a new match of distance dist1 + 1
XZE_HD void lzmaenc_match(LzmaEnc& e, uint16_t* probs, uint32_t pos, uint32_t dist1, uint32_t len)
{
    const uint32_t ps = pos & 3;
    xzrc_bit(e.rc, probs + kPIsMatch + (e.state << 4) + ps, 1);
    xzrc_bit(e.rc, probs + kPIsRep + e.state, 0);
    lzmaenc_len(e, probs + kPLen, len, ps);
    e.state = e.state < 7 ? 7 : 10;
    const uint32_t slot = lzmaenc_dist_slot(dist1);
    xzrc_tree(e.rc, probs + kPPosSlot + ((len < 6 ? len - 2 : 3) << 6), 6, slot);
    if (slot >= 4) {
        const uint32_t nb = (slot >> 1) - 1;
        const uint32_t base = (2 | (slot & 1)) << nb;
        const uint32_t rest = dist1 - base;
        if (slot < 14) {
            xzrc_tree_rev(e.rc, probs + kPSpecPos + base - slot - 1, nb, rest);
        } else {
            xzrc_direct(e.rc, rest >> 4, nb - 4);
            xzrc_tree_rev(e.rc, probs + kPAlign, 4, rest & 15);
        }
    }
    e.rep3 = e.rep2;
    e.rep2 = e.rep1;
    e.rep1 = e.rep0;
    e.rep0 = dist1;
}

// a match of rep distance k
XZE_HD void lzmaenc_rep(LzmaEnc& e, uint16_t* probs, uint32_t pos, uint32_t k, uint32_t len)
{
    const uint32_t ps = pos & 3;
    xzrc_bit(e.rc, probs + kPIsMatch + (e.state << 4) + ps, 1);
    xzrc_bit(e.rc, probs + kPIsRep + e.state, 1);
    if (k == 0) {
        xzrc_bit(e.rc, probs + kPIsRepG0 + e.state, 0);
        xzrc_bit(e.rc, probs + kPIsRep0Long + (e.state << 4) + ps, 1);
    } else {
        xzrc_bit(e.rc, probs + kPIsRepG0 + e.state, 1);
        if (k == 1) { // (a branch a distance, no select among the four: they stay in registers on the device)
            xzrc_bit(e.rc, probs + kPIsRepG1 + e.state, 0);
            const uint32_t dist = e.rep1;
            e.rep1 = e.rep0;
            e.rep0 = dist;
        } else if (k == 2) {
            xzrc_bit(e.rc, probs + kPIsRepG1 + e.state, 1);
            xzrc_bit(e.rc, probs + kPIsRepG2 + e.state, 0);
            const uint32_t dist = e.rep2;
            e.rep2 = e.rep1;
            e.rep1 = e.rep0;
            e.rep0 = dist;
        } else {
            xzrc_bit(e.rc, probs + kPIsRepG1 + e.state, 1);
            xzrc_bit(e.rc, probs + kPIsRepG2 + e.state, 1);
            const uint32_t dist = e.rep3;
            e.rep3 = e.rep2;
            e.rep2 = e.rep1;
            e.rep1 = e.rep0;
            e.rep0 = dist;
        }
    }
    lzmaenc_len(e, probs + kPRepLen, len, ps);
    e.state = e.state < 7 ? 8 : 11;
}

XZE_HD void lzmaenc_short_rep(LzmaEnc& e, uint16_t* probs, uint32_t pos)
{
    const uint32_t ps = pos & 3;
    xzrc_bit(e.rc, probs + kPIsMatch + (e.state << 4) + ps, 1);
    xzrc_bit(e.rc, probs + kPIsRep + e.state, 1);
    xzrc_bit(e.rc, probs + kPIsRepG0 + e.state, 0);
    xzrc_bit(e.rc, probs + kPIsRep0Long + (e.state << 4) + ps, 0);
    e.state = e.state < 7 ? 9 : 11;
}

// ---- a chunk ---------------------------------------------------------------------------------------------------------------

// What the encoder tells about the operations it chose (the host harness counts them; the kernel passes NoEncOps).
struct NoEncOps {
    XZE_HD void lit(uint32_t) {}
    XZE_HD void short_rep(uint32_t) {}
    XZE_HD void match(uint32_t, uint32_t, uint32_t) {} // position, distance, length
    XZE_HD void rep(uint32_t, uint32_t, uint32_t) {}   // position, k, length
};

XZE_HD bool xzenc_is_lzma(uint32_t csize, uint32_t usize) { return 6 + (uint64_t)csize < 3 + (uint64_t)usize && csize <= 65536; }

// Codes the chunk [cs, ce) of the Block blk into out[0 .. cap): the chunk's result, its csize or kXzEncStored.  cand: the
// Block's candidates (xzenc_find), indexed by Block position; probs: kXzEncProbs entries, all kLzmaProbInit.  The coder
// gives up as soon as its output can no longer be smaller than the bytes themselves.
template <class OPS>
XZE_HD uint32_t xzenc_chunk(const uint8_t* blk, uint32_t cs, uint32_t ce, const uint32_t* cand, uint16_t* probs, uint8_t* out, uint32_t cap,
                           OPS& ops)
{
    const uint32_t usize = ce - cs;
    LzmaEnc e;
    xzrc_init(e.rc, out, cap);
    e.state = 0;
    e.rep0 = e.rep1 = e.rep2 = e.rep3 = 0;
    uint32_t pos = cs;
    while (pos < ce) {
        if (e.rc.n + e.rc.cache_size >= usize) return kXzEncStored; // (the flush adds four bytes at least)
        const uint32_t maxlen = ce - pos < kLzmaMatchMax ? ce - pos : kLzmaMatchMax;
        // the rep distances first; none before the Block's first byte
        uint32_t rep_len = 0, rep_k = 0;
        bool rep0_byte = false;
        if (pos > 0) {
            const uint32_t d0 = e.rep0 + 1, d1 = e.rep1 + 1, d2 = e.rep2 + 1, d3 = e.rep3 + 1;
            if (d0 <= pos) {
                rep0_byte = blk[pos - d0] == blk[pos];
                rep_len = xzenc_common(blk + pos - d0, blk + pos, maxlen);
            }
            const uint32_t l1 = d1 <= pos ? xzenc_common(blk + pos - d1, blk + pos, maxlen) : 0;
            if (l1 > rep_len) { rep_len = l1; rep_k = 1; }
            const uint32_t l2 = d2 <= pos ? xzenc_common(blk + pos - d2, blk + pos, maxlen) : 0;
            if (l2 > rep_len) { rep_len = l2; rep_k = 2; }
            const uint32_t l3 = d3 <= pos ? xzenc_common(blk + pos - d3, blk + pos, maxlen) : 0;
            if (l3 > rep_len) { rep_len = l3; rep_k = 3; }
        }
        const uint32_t m = cand[pos];
        const uint32_t mlen = xzenc_cand_len(m);
        if (rep_len >= 2 && rep_len + 1 >= mlen) { // a rep beats a new match at most one byte longer
            ops.rep(pos, rep_k, rep_len);
            lzmaenc_rep(e, probs, pos, rep_k, rep_len);
            pos += rep_len;
            continue;
        }
        // one step of lazy evaluation: a longer match at the next position is worth a literal here
        if (mlen >= 2 && !(pos + 1 < ce && xzenc_cand_len(cand[pos + 1]) > mlen)) {
            ops.match(pos, xzenc_cand_dist1(m) + 1, mlen);
            lzmaenc_match(e, probs, pos, xzenc_cand_dist1(m), mlen);
            pos += mlen;
            continue;
        }
        if (rep0_byte) {
            ops.short_rep(pos);
            lzmaenc_short_rep(e, probs, pos);
        } else {
            ops.lit(e.state >= 7);
            lzmaenc_literal(e, probs, blk, pos, pos ? blk[pos - 1] : 0);
        }
        ++pos;
    }
    const uint32_t csize = xzrc_finish(e.rc);
    return xzenc_is_lzma(csize, usize) ? csize : kXzEncStored;
}

// A chunk's header into p: 6 bytes for LZMA (res = csize), 3 for an uncompressed chunk (res = kXzEncStored).  first: the
// Block's first chunk resets the dictionary; every chunk resets the state and sends the properties.
XZE_HD uint32_t xzenc_chunk_header(uint8_t* p, bool first, uint32_t usize, uint32_t res)
{
    if (res == kXzEncStored) {
        p[0] = first ? 0x01 : 0x02;
        p[1] = (uint8_t)((usize - 1) >> 8);
        p[2] = (uint8_t)(usize - 1);
        return 3;
    }
    p[0] = (uint8_t)((first ? 0xE0 : 0xC0) | ((usize - 1) >> 16));
    p[1] = (uint8_t)((usize - 1) >> 8);
    p[2] = (uint8_t)(usize - 1);
    p[3] = (uint8_t)((res - 1) >> 8);
    p[4] = (uint8_t)(res - 1);
    p[5] = (uint8_t)kXzEncProps;
    return 6;
}
// what a chunk takes in its Block's data: header and body
XZE_HD uint32_t xzenc_chunk_bytes(uint32_t usize, uint32_t res) { return res == kXzEncStored ? 3 + usize : 6 + res; }
// a result the kernel may report for a chunk of usize bytes
XZE_HD bool xzenc_res_valid(uint32_t usize, uint32_t res) { return res == kXzEncStored || (res >= 5 && xzenc_is_lzma(res, usize)); }

// ---- level 1: several candidates a position, prices, a shortest-path parse ------------------------------
//
// The chunk's bytes stay a pure function of (the Block's bytes, the chunk's bounds, the level).  xzenc_chunk_priced is ONE
// function for the host model and the kernel; what differs is LN, the lanes: the kernel's 256 threads with a barrier, or
// a loop over 256 lane numbers on the host, in ascending or descending order.  The contract that keeps the two byte for
// byte equal:
//   - A window of at most kXzEncWindow positions is parsed at a time, with prices taken from the probabilities as they
//     stand at its start.  Node t is "t bytes into the window"; the edges out of node cur are, in this order of index:
//     0 the literal, 1 the short rep, 2..5 rep0..rep3, 6..6+K-1 the candidates nearest first; a rep or candidate of
//     length n gives an edge of every length 2..n, cut at the chunk's end and at the window's.
//   - The edges of ONE node are relaxed side by side, a lane a target: lane i owns the targets cur + 2 + i and
//     cur + 2 + i + 256, lane 0 the target cur + 1 as well.  Only the owner writes a target's node, so no two lanes meet.
//     Among the edges into one target from one node the lowest price wins, and of equal prices the lower edge index; an
//     edge from a later node replaces what an earlier node left only when it is strictly cheaper.  No step depends on
//     the order in which the lanes run.
//   - The window closes where every path has come together (no edge reaches past the node in hand), when it is full, or
//     in front of a position where a match of 273 bytes starts; such a match at the window's first position is taken as
//     it is, the lowest rep that has it before a candidate.
//   - Then lane 0 walks the chosen edges back, codes them with the lzmaenc_* routines above (the probabilities adapt),
//     and the next window opens.  The give-up of xzenc_chunk and xzenc_is_lzma hold as at level 0.
constexpr uint32_t kXzEncDepthHigh = 32;  // chain links examined per position at level 1
constexpr uint32_t kXzEncCands = 4;       // K: candidates kept per position
constexpr uint32_t kXzEncWindow = 1024;   // W: positions of a window
constexpr uint32_t kXzEncLanes = 256;     // lanes that relax a node's edges
constexpr uint32_t kXzEncLevelMax = 1;
constexpr uint32_t kXzEncPriceInf = 1u << 30;
constexpr uint32_t kXzEncSlots = 44;      // distance slots a Block of at most 4 MiB can need
enum : uint32_t { kXzEdgeLit = 0, kXzEdgeShortRep = 1, kXzEdgeRep = 2, kXzEdgeMatch = 6 };

// Up to K candidates at position p, into out[0 .. K): lengths strictly rising and for each length the nearest distance
// (the chain is walked nearest first, kXzEncDepthHigh links), packed as xzenc_find packs one, 0 behind the last.  Of
// more than K the longest K are kept.  Every compare is cut at the chunk's end.
XZE_HD void xzenc_find_set(const uint8_t* blk, const uint32_t* prev, uint32_t p, uint32_t ce, uint32_t* out)
{
    static_assert(kXzEncCands == 4, "four names, not an array: they stay in registers on the device");
    uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0, n = 0;
    const uint32_t maxlen = ce - p < kLzmaMatchMax ? ce - p : kLzmaMatchMax;
    if (maxlen >= 2) {
        uint32_t best_len = 1;
        uint32_t c = prev[p];
        for (uint32_t d = 0; d < kXzEncDepthHigh && c < p; ++d) { // (kXzEncNone fails c < p)
            const uint32_t l = xzenc_common(blk + c, blk + p, maxlen);
            if (l > best_len) {
                best_len = l;
                a0 = a1; a1 = a2; a2 = a3;
                a3 = l << 22 | (p - c - 1);
                if (n < kXzEncCands) ++n;
                if (l == maxlen) break;
            }
            c = prev[c];
        }
    }
    for (uint32_t i = n; i < kXzEncCands; ++i) { a0 = a1; a1 = a2; a2 = a3; a3 = 0; } // to the front
    out[0] = a0; out[1] = a1; out[2] = a2; out[3] = a3;
}

// round(-16 log2(p / 2048)) for 1 <= p < 2048, in integers: the whole part of log2 from the leading bit, five more bits
// by squaring (the last one rounds)
XZE_HD uint32_t xzenc_price_of(uint32_t p)
{
    const uint32_t msb = 31 - (uint32_t)__builtin_clz(p);
    uint64_t x = (uint64_t)p << (31 - msb); // p / 2^msb in [1, 2), 31 bits behind the point
    uint32_t l32 = msb;
    for (int i = 0; i < 5; ++i) {
        x = (x * x) >> 31;
        l32 <<= 1;
        if (x >> 32) { l32 |= 1; x >>= 1; }
    }
    return (705 - 2 * l32) >> 2; // 16 * 11 - (l32 + 1/2) / 2, to the nearest
}

struct XzEncNode {
    uint32_t price;
    uint32_t dist;   // a match's distance - 1
    uint16_t len;    // of the edge that arrives here: the node it left is len in front
    uint8_t kind;    // kXzEdge*: for a rep kXzEdgeRep + k
    uint8_t state;   // the coder's here, and its rep distances: set when the node is visited
    uint32_t rep[4];
};
// What the parse keeps beside the probabilities: LDS in the kernel.  28 700 + 2 050 + 256 + 4 352 + 352 + 32 + 8 bytes.
struct XzEncWork {
    XzEncNode node[kXzEncWindow + 1];
    uint16_t next[kXzEncWindow + 1];                          // lane 0's: the chosen edges, forwards
    uint16_t ptab[128];                                       // a bit's price by probability >> 4
    uint16_t lenp[2 * 4 * (kLzmaMatchMax - 1)];               // [new match, rep][pos_state][len - 2]
    uint16_t slotp[4 * kXzEncSlots];                          // [len state][slot]
    uint16_t alignp[16];
    uint32_t flag, res;                                       // lane 0 tells the others: gave up; the chunk's result
};

XZE_HD uint32_t xzp_bit(const uint16_t* ptab, uint32_t prob, uint32_t bit) { return ptab[((bit ? 2048 - prob : prob) >> 4) & 127]; }
XZE_HD uint32_t xzp_tree(const uint16_t* ptab, const uint16_t* p, uint32_t bits, uint32_t value)
{
    uint32_t m = 1, sum = 0;
    for (uint32_t i = bits; i-- > 0;) {
        const uint32_t b = (value >> i) & 1;
        sum += xzp_bit(ptab, p[m], b);
        m = (m << 1) | b;
    }
    return sum;
}
XZE_HD uint32_t xzp_tree_rev(const uint16_t* ptab, const uint16_t* p, uint32_t bits, uint32_t value)
{
    uint32_t m = 1, sum = 0;
    for (uint32_t i = 0; i < bits; ++i) {
        const uint32_t b = (value >> i) & 1;
        sum += xzp_bit(ptab, p[m], b);
        m = (m << 1) | b;
    }
    return sum;
}
// what lzmaenc_len would pay; p: probs + kPLen or kPRepLen
XZE_HD uint32_t xzp_len(const uint16_t* ptab, const uint16_t* p, uint32_t len, uint32_t pos_state)
{
    const uint32_t l = len - 2;
    if (l < 8) return xzp_bit(ptab, p[kLenChoice], 0) + xzp_tree(ptab, p + kLenLow + (pos_state << 3), 3, l);
    if (l < 16) return xzp_bit(ptab, p[kLenChoice], 1) + xzp_bit(ptab, p[kLenChoice2], 0) + xzp_tree(ptab, p + kLenMid + (pos_state << 3), 3, l - 8);
    return xzp_bit(ptab, p[kLenChoice], 1) + xzp_bit(ptab, p[kLenChoice2], 1) + xzp_tree(ptab, p + kLenHigh, 8, l - 16);
}
// what lzmaenc_literal would pay for the byte at pos in state `state` with rep0
XZE_HD uint32_t xzp_literal(const uint16_t* ptab, const uint16_t* probs, const uint8_t* blk, uint32_t pos, uint32_t state, uint32_t rep0)
{
    const uint32_t b = blk[pos];
    const uint16_t* p = probs + kLzmaLitBase + 0x300u * ((pos ? blk[pos - 1] : 0u) >> 5);
    if (state < 7) return xzp_tree(ptab, p, 8, b);
    uint32_t mb = blk[pos - rep0 - 1], offs = 0x100, sym = 1, sum = 0;
    for (uint32_t i = 8; i-- > 0;) {
        mb <<= 1;
        const uint32_t mbit = mb & offs;
        const uint32_t bit = (b >> i) & 1;
        sum += xzp_bit(ptab, p[offs + mbit + sym], bit);
        sym = (sym << 1) | bit;
        offs &= bit ? mbit : ~mbit;
    }
    return sum;
}
// what lzmaenc_match would pay for the distance dist1 + 1 behind a length of len, from the tables
XZE_HD uint32_t xzp_dist(const XzEncWork& w, const uint16_t* probs, uint32_t dist1, uint32_t len)
{
    const uint32_t slot = lzmaenc_dist_slot(dist1);
    uint32_t sum = w.slotp[(len < 6 ? len - 2 : 3) * kXzEncSlots + slot];
    if (slot >= 4) {
        const uint32_t nb = (slot >> 1) - 1;
        const uint32_t base = (2 | (slot & 1)) << nb;
        const uint32_t rest = dist1 - base;
        if (slot < 14) sum += xzp_tree_rev(w.ptab, probs + kPSpecPos + base - slot - 1, nb, rest);
        else sum += 16 * (nb - 4) + w.alignp[rest & 15];
    }
    return sum;
}
// entry i of the tables behind ptab, i < kXzEncTableEntries: lengths, slots, align
constexpr uint32_t kXzEncLenEntries = 2 * 4 * (kLzmaMatchMax - 1);
constexpr uint32_t kXzEncTableEntries = kXzEncLenEntries + 4 * kXzEncSlots + 16;
XZE_HD void xzenc_table_entry(XzEncWork& w, const uint16_t* probs, uint32_t i)
{
    if (i < kXzEncLenEntries) {
        const uint32_t which = i / (4 * (kLzmaMatchMax - 1)), r = i % (4 * (kLzmaMatchMax - 1));
        w.lenp[i] = (uint16_t)xzp_len(w.ptab, probs + (which ? kPRepLen : kPLen), 2 + r % (kLzmaMatchMax - 1), r / (kLzmaMatchMax - 1));
    } else if (i < kXzEncLenEntries + 4 * kXzEncSlots) {
        const uint32_t j = i - kXzEncLenEntries;
        w.slotp[j] = (uint16_t)xzp_tree(w.ptab, probs + kPPosSlot + ((j / kXzEncSlots) << 6), 6, j % kXzEncSlots);
    } else {
        const uint32_t j = i - kXzEncLenEntries - 4 * kXzEncSlots;
        w.alignp[j] = (uint16_t)xzp_tree_rev(w.ptab, probs + kPAlign, 4, j);
    }
}

// the coder's state and rep distances behind an edge
XZE_HD void xzenc_apply(uint32_t kind, uint32_t dist, uint32_t& s, uint32_t& r0, uint32_t& r1, uint32_t& r2, uint32_t& r3)
{
    if (kind == kXzEdgeLit) {
        s = s < 4 ? 0 : s < 10 ? s - 3 : s - 6;
    } else if (kind == kXzEdgeShortRep) {
        s = s < 7 ? 9 : 11;
    } else if (kind == kXzEdgeMatch) {
        r3 = r2; r2 = r1; r1 = r0; r0 = dist;
        s = s < 7 ? 7 : 10;
    } else {
        const uint32_t k = kind - kXzEdgeRep;
        if (k == 1) { const uint32_t d = r1; r1 = r0; r0 = d; }
        else if (k == 2) { const uint32_t d = r2; r2 = r1; r1 = r0; r0 = d; }
        else if (k == 3) { const uint32_t d = r3; r3 = r2; r2 = r1; r1 = r0; r0 = d; }
        s = s < 7 ? 8 : 11;
    }
}

// The lanes of the host model: a loop.  first(): lane 0's part runs once; sync(): the kernel's barrier.
struct XzEncHostLanes {
    bool descending = false;
    template <class F> void each(F&& f)
    {
        if (!descending) for (uint32_t i = 0; i < kXzEncLanes; ++i) f(i);
        else for (uint32_t i = kXzEncLanes; i-- > 0;) f(i);
    }
    bool first() const { return true; }
    void sync() {}
};

// xzenc_chunk at level 1.  cand: kXzEncCands words a Block position (xzenc_find_set); w: scratch, any contents.  Every
// lane calls it with the same arguments and gets the same result; only lane 0 writes out.
template <class OPS, class LN>
XZE_HD uint32_t xzenc_chunk_priced(const uint8_t* blk, uint32_t cs, uint32_t ce, const uint32_t* cand, uint16_t* probs, XzEncWork& w, uint8_t* out,
                                  uint32_t cap, OPS& ops, LN& ln)
{
    const uint32_t usize = ce - cs;
    LzmaEnc e; // (lane 0's is the coder; the others carry state and reps along, which every lane derives alike)
    xzrc_init(e.rc, out, cap);
    e.state = 0;
    e.rep0 = e.rep1 = e.rep2 = e.rep3 = 0;
    ln.each([&](uint32_t lane) {
        if (lane < 128) w.ptab[lane] = (uint16_t)xzenc_price_of(16 * lane + 8);
    });
    uint32_t pos = cs, st = 0, w0 = 0, w1 = 0, w2 = 0, w3 = 0; // the window's start: position, state, reps
    while (pos < ce) {
        const uint32_t wmax = ce - pos < kXzEncWindow ? ce - pos : kXzEncWindow;
        if (ln.first()) {
            XzEncNode& z = w.node[0];
            z.price = 0; z.dist = 0; z.len = 0; z.kind = 0;
            z.state = (uint8_t)st;
            z.rep[0] = w0; z.rep[1] = w1; z.rep[2] = w2; z.rep[3] = w3;
        }
        uint32_t len_end = 0, cur = 0;
        uint32_t s = st, r0 = w0, r1 = w1, r2 = w2, r3 = w3; // the node in hand
        for (;; ++cur) {
            ln.sync(); // what the lanes left in the nodes (and, at a window's start, lane 0 in the probabilities) is there
            uint32_t price = 0;
            if (cur > 0) {
                const XzEncNode& z = w.node[cur];
                const XzEncNode& f = w.node[cur - z.len];
                price = z.price;
                s = f.state; r0 = f.rep[0]; r1 = f.rep[1]; r2 = f.rep[2]; r3 = f.rep[3];
                xzenc_apply(z.kind, z.dist, s, r0, r1, r2, r3);
                if (cur == len_end) break;
                if (ln.first()) {
                    XzEncNode& zz = w.node[cur];
                    zz.state = (uint8_t)s;
                    zz.rep[0] = r0; zz.rep[1] = r1; zz.rep[2] = r2; zz.rep[3] = r3;
                }
            }
            const uint32_t p = pos + cur, ps = p & 3;
            uint32_t maxlen = ce - p < kLzmaMatchMax ? ce - p : kLzmaMatchMax;
            if (maxlen > wmax - cur) maxlen = wmax - cur;
            // what leaves this node: the reps (none before the Block's first byte) and the candidates, cut to maxlen
            uint32_t l0 = 0, l1 = 0, l2 = 0, l3 = 0;
            bool rep0_byte = false;
            if (p > 0) {
                if (r0 + 1 <= p) {
                    rep0_byte = blk[p - r0 - 1] == blk[p];
                    if (maxlen >= 2) l0 = xzenc_common(blk + p - r0 - 1, blk + p, maxlen);
                }
                if (maxlen >= 2) {
                    if (r1 + 1 <= p) l1 = xzenc_common(blk + p - r1 - 1, blk + p, maxlen);
                    if (r2 + 1 <= p) l2 = xzenc_common(blk + p - r2 - 1, blk + p, maxlen);
                    if (r3 + 1 <= p) l3 = xzenc_common(blk + p - r3 - 1, blk + p, maxlen);
                }
            }
            const uint32_t* cp = cand + (size_t)p * kXzEncCands;
            const uint32_t c0 = cp[0], c1 = cp[1], c2 = cp[2], c3 = cp[3];
            uint32_t m0 = xzenc_cand_len(c0), m1 = xzenc_cand_len(c1), m2 = xzenc_cand_len(c2), m3 = xzenc_cand_len(c3);
            const bool maximal = m0 == kLzmaMatchMax || m1 == kLzmaMatchMax || m2 == kLzmaMatchMax || m3 == kLzmaMatchMax ||
                                 l0 == kLzmaMatchMax || l1 == kLzmaMatchMax || l2 == kLzmaMatchMax || l3 == kLzmaMatchMax;
            if (m0 > maxlen) m0 = maxlen;
            if (m1 > maxlen) m1 = maxlen;
            if (m2 > maxlen) m2 = maxlen;
            if (m3 > maxlen) m3 = maxlen;
            if (maxlen < 2) m0 = m1 = m2 = m3 = 0;
            uint32_t longest = l0;
            if (l1 > longest) longest = l1;
            if (l2 > longest) longest = l2;
            if (l3 > longest) longest = l3;
            if (m0 > longest) longest = m0;
            if (m1 > longest) longest = m1;
            if (m2 > longest) longest = m2;
            if (m3 > longest) longest = m3;
            if (longest < 2) longest = 0;
            if (maximal && maxlen == kLzmaMatchMax) {
                if (cur > 0) { // the window closes in front of it
                    len_end = cur;
                    break;
                }
                // the window's first position: the match as it is
                uint32_t kind = kXzEdgeMatch, dist = 0;
                if (l0 == kLzmaMatchMax) kind = kXzEdgeRep;
                else if (l1 == kLzmaMatchMax) kind = kXzEdgeRep + 1;
                else if (l2 == kLzmaMatchMax) kind = kXzEdgeRep + 2;
                else if (l3 == kLzmaMatchMax) kind = kXzEdgeRep + 3;
                else dist = xzenc_cand_dist1(m0 == kLzmaMatchMax ? c0 : m1 == kLzmaMatchMax ? c1 : m2 == kLzmaMatchMax ? c2 : c3);
                if (ln.first()) {
                    XzEncNode& z = w.node[kLzmaMatchMax];
                    z.price = 0; z.dist = dist; z.len = (uint16_t)kLzmaMatchMax; z.kind = (uint8_t)kind;
                }
                xzenc_apply(kind, dist, s, r0, r1, r2, r3);
                len_end = kLzmaMatchMax;
                break;
            }
            if (cur == 0 && longest) { // the tables, from the probabilities as they stand now (a window of one byte needs none)
                ln.each([&](uint32_t lane) {
                    for (uint32_t i = lane; i < kXzEncTableEntries; i += kXzEncLanes) xzenc_table_entry(w, probs, i);
                });
                ln.sync();
            }
            const uint32_t old_end = len_end;
            if (cur + (longest ? longest : 1) > len_end) len_end = cur + (longest ? longest : 1);
            const uint32_t pm1 = price + xzp_bit(w.ptab, probs[kPIsMatch + (s << 4) + ps], 1);
            const uint32_t prep = pm1 + xzp_bit(w.ptab, probs[kPIsRep + s], 1);
            const uint32_t pg0 = xzp_bit(w.ptab, probs[kPIsRepG0 + s], 0);
            if (ln.first()) { // edges 0 and 1, to the next node
                uint32_t best = cur + 1 <= old_end ? w.node[cur + 1].price : kXzEncPriceInf;
                uint32_t kind = 0xff;
                const uint32_t plit = price + xzp_bit(w.ptab, probs[kPIsMatch + (s << 4) + ps], 0) + xzp_literal(w.ptab, probs, blk, p, s, r0);
                if (plit < best) { best = plit; kind = kXzEdgeLit; }
                if (rep0_byte) {
                    const uint32_t psr = prep + pg0 + xzp_bit(w.ptab, probs[kPIsRep0Long + (s << 4) + ps], 0);
                    if (psr < best) { best = psr; kind = kXzEdgeShortRep; }
                }
                if (kind != 0xff) {
                    XzEncNode& z = w.node[cur + 1];
                    z.price = best; z.dist = 0; z.len = 1; z.kind = (uint8_t)kind;
                }
            }
            if (longest) {
                const uint32_t pg0_1 = xzp_bit(w.ptab, probs[kPIsRepG0 + s], 1);
                const uint32_t pg1_1 = xzp_bit(w.ptab, probs[kPIsRepG1 + s], 1);
                const uint32_t b0 = prep + pg0 + xzp_bit(w.ptab, probs[kPIsRep0Long + (s << 4) + ps], 1);
                const uint32_t b1 = prep + pg0_1 + xzp_bit(w.ptab, probs[kPIsRepG1 + s], 0);
                const uint32_t b2 = prep + pg0_1 + pg1_1 + xzp_bit(w.ptab, probs[kPIsRepG2 + s], 0);
                const uint32_t b3 = prep + pg0_1 + pg1_1 + xzp_bit(w.ptab, probs[kPIsRepG2 + s], 1);
                const uint32_t pnew = pm1 + xzp_bit(w.ptab, probs[kPIsRep + s], 0);
                const uint16_t* lrep = w.lenp + (4 + ps) * (kLzmaMatchMax - 1);
                const uint16_t* lnew = w.lenp + ps * (kLzmaMatchMax - 1);
                ln.each([&](uint32_t lane) {
                    for (uint32_t L = 2 + lane; L <= longest; L += kXzEncLanes) {
                        const uint32_t t = cur + L;
                        uint32_t best = t <= old_end ? w.node[t].price : kXzEncPriceInf;
                        uint32_t kind = 0xff, dist = 0;
                        const uint32_t lr = lrep[L - 2], lm = pnew + lnew[L - 2];
                        if (l0 >= L && b0 + lr < best) { best = b0 + lr; kind = kXzEdgeRep; }
                        if (l1 >= L && b1 + lr < best) { best = b1 + lr; kind = kXzEdgeRep + 1; }
                        if (l2 >= L && b2 + lr < best) { best = b2 + lr; kind = kXzEdgeRep + 2; }
                        if (l3 >= L && b3 + lr < best) { best = b3 + lr; kind = kXzEdgeRep + 3; }
                        if (m0 >= L) { const uint32_t q = lm + xzp_dist(w, probs, xzenc_cand_dist1(c0), L); if (q < best) { best = q; kind = kXzEdgeMatch; dist = xzenc_cand_dist1(c0); } }
                        if (m1 >= L) { const uint32_t q = lm + xzp_dist(w, probs, xzenc_cand_dist1(c1), L); if (q < best) { best = q; kind = kXzEdgeMatch; dist = xzenc_cand_dist1(c1); } }
                        if (m2 >= L) { const uint32_t q = lm + xzp_dist(w, probs, xzenc_cand_dist1(c2), L); if (q < best) { best = q; kind = kXzEdgeMatch; dist = xzenc_cand_dist1(c2); } }
                        if (m3 >= L) { const uint32_t q = lm + xzp_dist(w, probs, xzenc_cand_dist1(c3), L); if (q < best) { best = q; kind = kXzEdgeMatch; dist = xzenc_cand_dist1(c3); } }
                        if (kind != 0xff) {
                            XzEncNode& z = w.node[t];
                            z.price = best; z.dist = dist; z.len = (uint16_t)L; z.kind = (uint8_t)kind;
                        }
                    }
                });
            }
        }
        // lane 0: the chosen edges forwards, coded; (s, r0..r3) is the state behind them on every lane
        if (ln.first()) {
            for (uint32_t t = len_end; t;) {
                const uint32_t L = w.node[t].len;
                w.next[t - L] = (uint16_t)L;
                t -= L;
            }
            uint32_t gave = 0;
            for (uint32_t t = 0; t < len_end;) {
                if (e.rc.n + e.rc.cache_size >= usize) { // (the flush adds four bytes at least)
                    gave = 1;
                    break;
                }
                const uint32_t L = w.next[t], q = pos + t;
                const XzEncNode& z = w.node[t + L];
                if (z.kind == kXzEdgeLit) {
                    ops.lit(e.state >= 7);
                    lzmaenc_literal(e, probs, blk, q, q ? blk[q - 1] : 0);
                } else if (z.kind == kXzEdgeShortRep) {
                    ops.short_rep(q);
                    lzmaenc_short_rep(e, probs, q);
                } else if (z.kind == kXzEdgeMatch) {
                    ops.match(q, z.dist + 1, L);
                    lzmaenc_match(e, probs, q, z.dist, L);
                } else {
                    ops.rep(q, z.kind - kXzEdgeRep, L);
                    lzmaenc_rep(e, probs, q, z.kind - kXzEdgeRep, L);
                }
                t += L;
            }
            w.flag = gave;
        }
        ln.sync();
        if (w.flag) return kXzEncStored;
        pos += len_end;
        st = s; w0 = r0; w1 = r1; w2 = r2; w3 = r3;
    }
    if (ln.first()) {
        const uint32_t csize = xzrc_finish(e.rc);
        w.res = xzenc_is_lzma(csize, usize) ? csize : kXzEncStored;
    }
    ln.sync();
    return w.res;
}

// ---- the container (host only) -------------------------------------------------------------------------------------------

// 0 = the default; a multiple of 64 KiB from 64 KiB to kXzEncBlockMax
inline bool xzenc_block_size(uint64_t* block_size)
{
    if (*block_size == 0) *block_size = kXzEncBlockDefault;
    return *block_size >= kXzEncChunk && *block_size <= kXzEncBlockMax && *block_size % kXzEncChunk == 0;
}
// the smallest encodable dictionary that holds a Block: xz_dict_size run backwards
inline uint32_t xzenc_dict_byte(uint64_t block_size)
{
    uint32_t b = 0;
    while (b < 40 && xz_dict_size(b) < block_size) ++b;
    return b;
}
inline uint32_t xzenc_vli(uint8_t* p, uint64_t v)
{
    uint32_t n = 0;
    while (v >= 0x80) {
        p[n++] = (uint8_t)(v | 0x80);
        v >>= 7;
    }
    p[n++] = (uint8_t)v;
    return n;
}
inline void xzenc_le32(uint8_t* p, uint32_t v)
{
    for (int k = 0; k < 4; ++k) p[k] = (uint8_t)(v >> (8 * k));
}
inline void xzenc_le64(uint8_t* p, uint64_t v)
{
    for (int k = 0; k < 8; ++k) p[k] = (uint8_t)(v >> (8 * k));
}
constexpr uint32_t kXzEncStreamHeader = 12, kXzEncBlockHeaderMax = 32, kXzEncCheck = 8; // (CRC-64's size: the default Check)
constexpr uint32_t kXzEncCheckMax = 32;

// the Checks this side writes: what the install side reads
inline bool xzenc_check_valid(uint32_t check)
{
    return check == kXzCheckNone || check == kXzCheckCrc32 || check == kXzCheckCrc64 || check == kXzCheckSha256;
}
// the bytes of a Block's Check field
inline uint32_t xzenc_check_size(uint32_t check) { return check == kXzCheckNone ? 0 : check == kXzCheckCrc32 ? 4 : check == kXzCheckCrc64 ? 8 : 32; }

inline void xzenc_stream_header(uint8_t* p, uint32_t check = kXzCheckCrc64)
{
    static const uint8_t magic[6] = {0xFD, '7', 'z', 'X', 'Z', 0};
    memcpy(p, magic, 6);
    p[6] = 0;
    p[7] = (uint8_t)check;
    xzenc_le32(p + 8, xz_crc32(p + 6, 2));
}
// The filters a Block names in front of LZMA2, the header's first filter first: none, one BCJ filter (a plain id converts: the
// `filter` of DESIGN.md sec. 25), or up to three of Delta and the six BCJ filters (sec. 29).  param: Delta's distance; a BCJ
// filter is named without properties, its start_offset 0.
struct XzEncChain {
    uint32_t n = 0;
    uint32_t id[3] = {0, 0, 0};
    uint32_t param[3] = {0, 0, 0};
    XzEncChain() = default;
    bool plain = false; // made from a plain id: held to the three ids the `filter` field takes
    XzEncChain(uint32_t filter) : n(filter ? 1 : 0), plain(true) { id[0] = filter; }
    explicit operator bool() const { return n != 0; }
    uint32_t first() const { return n ? id[0] : 0; }
};
// a chain this side writes: every filter one liblzma knows, a distance of 1 .. 256, no parameter on a BCJ filter
inline bool xzenc_chain_valid(const XzEncChain& c)
{
    if (c.n > 3) return false;
    if (c.plain) return c.id[0] == 0 || bcj_filter_valid(c.id[0]);
    for (uint32_t k = 0; k < c.n; ++k)
        if (!xz_filter_valid(c.id[k]) || (c.id[k] == kXzDelta ? !delta_dist_valid(c.param[k]) : c.param[k] != 0)) return false;
    return true;
}
// the chain applied to a Block on one thread, in place, as the kernels apply it stage by stage
inline void xzenc_chain_apply(const XzEncChain& c, uint8_t* b, uint64_t len)
{
    for (uint32_t k = 0; k < c.n; ++k) {
        if (c.id[k] == kXzDelta) delta_block(true, b, len, c.param[k]);
        else bcj_block(c.id[k], true, b, len, 0);
    }
}
// a Block header that states both sizes, into p (kXzEncBlockHeaderMax bytes of room): its size.  chain: the filters in front
// of LZMA2 -- Delta with its one property byte, a BCJ filter (bcj_core.h's ids) without properties
inline uint32_t xzenc_block_header(uint8_t* p, uint64_t csize, uint64_t usize, uint32_t dict_byte, const XzEncChain& chain = XzEncChain())
{
    uint32_t n = 2;
    p[1] = (uint8_t)(0xC0 | chain.n); // 1 + chain.n filters; compressed and uncompressed size present
    n += xzenc_vli(p + n, csize);
    n += xzenc_vli(p + n, usize);
    for (uint32_t k = 0; k < chain.n; ++k) {
        p[n++] = (uint8_t)chain.id[k];
        if (chain.id[k] == kXzDelta) {
            p[n++] = 0x01;
            p[n++] = (uint8_t)(chain.param[k] - 1);
        } else {
            p[n++] = 0x00;
        }
    }
    p[n++] = 0x21;
    p[n++] = 0x01;
    p[n++] = (uint8_t)dict_byte;
    while (n & 3) p[n++] = 0;
    p[0] = (uint8_t)((n + 4) / 4 - 1);
    xzenc_le32(p + n, xz_crc32(p, n));
    return n + 4;
}
inline uint32_t xzenc_block_header_size(uint64_t csize, uint64_t usize, const XzEncChain& chain = XzEncChain())
{
    uint8_t t[kXzEncBlockHeaderMax];
    return xzenc_block_header(t, csize, usize, 0, chain);
}
// the filters this side writes in front of LZMA2 through the `filter` field (0: none)
inline bool xzenc_filter_valid(uint32_t filter) { return filter == 0 || bcj_filter_valid(filter); }
struct XzEncRecord { uint64_t unpadded, usize; };
// the Index and the Stream footer behind the last Block
inline void xzenc_index_footer(const std::vector<XzEncRecord>& recs, std::vector<uint8_t>& out, uint32_t check = kXzCheckCrc64)
{
    const size_t i0 = out.size();
    uint8_t t[10];
    out.push_back(0);
    out.insert(out.end(), t, t + xzenc_vli(t, recs.size()));
    for (const XzEncRecord& r : recs) {
        out.insert(out.end(), t, t + xzenc_vli(t, r.unpadded));
        out.insert(out.end(), t, t + xzenc_vli(t, r.usize));
    }
    while ((out.size() - i0) & 3) out.push_back(0);
    xzenc_le32(t, xz_crc32(out.data() + i0, out.size() - i0));
    out.insert(out.end(), t, t + 4);
    const uint64_t isize = out.size() - i0;
    uint8_t f[12];
    xzenc_le32(f + 4, (uint32_t)(isize / 4 - 1));
    f[8] = 0;
    f[9] = (uint8_t)check;
    xzenc_le32(f, xz_crc32(f + 4, 6));
    f[10] = 'Y';
    f[11] = 'Z';
    out.insert(out.end(), f, f + 12);
}

// Where a Block's parts lie, from its chunks' results: dst[k] = chunk k's header, relative to the Block's first byte.
struct XzEncBlockLayout {
    uint32_t hdr = 0;       // the Block header's size
    uint64_t data = 0;      // the LZMA2 data with its end byte
    uint64_t check_at = 0;  // behind the Block Padding
    uint64_t total = 0;     // header, data, padding, Check
    uint64_t unpadded = 0;  // the Index record's
};
inline XzEncBlockLayout xzenc_block_layout(const uint32_t* res, uint32_t nch, uint64_t blen, uint64_t* dst, uint32_t check = kXzCheckCrc64,
                                           const XzEncChain& filter = XzEncChain())
{
    const uint32_t check_size = xzenc_check_size(check);
    XzEncBlockLayout L;
    uint64_t data = 0;
    for (uint32_t k = 0; k < nch; ++k) {
        const uint32_t usize = (uint32_t)std::min<uint64_t>(kXzEncChunk, blen - (uint64_t)k * kXzEncChunk);
        dst[k] = data;
        data += xzenc_chunk_bytes(usize, res[k]);
    }
    L.data = data + 1;
    L.hdr = xzenc_block_header_size(L.data, blen, filter);
    for (uint32_t k = 0; k < nch; ++k) dst[k] += L.hdr;
    L.unpadded = L.hdr + L.data + check_size;
    L.check_at = (L.hdr + L.data + 3) & ~3ull;
    L.total = L.check_at + check_size;
    return L;
}

// ---- the host model --------------------------------------------------------------------------------------------------------

// prev[p] for every position of the Block blk[0 .. blen); head: 1 << kXzEncHashBits entries of scratch
inline void xzenc_chains_host(const uint8_t* blk, uint32_t blen, uint32_t* prev, uint32_t* head)
{
    for (uint32_t i = 0; i < (1u << kXzEncHashBits); ++i) head[i] = kXzEncNone;
    for (uint32_t p = 0; p < blen; ++p) {
        if (p + 4 > blen) {
            prev[p] = kXzEncNone;
            continue;
        }
        const uint32_t h = xzenc_hash(xzenc_ld32(blk + p));
        prev[p] = head[h];
        head[h] = p;
    }
}

struct XzEncInfo {
    uint64_t chunks = 0, stored = 0;
    std::vector<uint32_t> res; // every chunk's result, in order
};

// One Block through the three steps, as the kernels leave their arrays: prev and cand (blen words each, Block-relative; at
// level 1 cand holds kXzEncCands words a position and the lanes run in the order lanes_descending says),
// res and dst (a word a chunk; dst relative to the Block's first byte) and slots (kXzEncSlot bytes a chunk: the coder's
// output, nothing else written).  head: 1 << kXzEncHashBits entries of scratch; probs: kXzEncProbs.
template <class OPS>
inline XzEncBlockLayout xzenc_block_stages(const uint8_t* blk, uint32_t blen, uint32_t* prev, uint32_t* cand, uint32_t* head, uint16_t* probs,
                                           uint32_t* res, uint64_t* dst, uint8_t* slots, OPS& ops, uint32_t check = kXzCheckCrc64,
                                           const XzEncChain& filter = XzEncChain(), uint32_t level = 0, bool lanes_descending = false)
{
    const uint32_t nch = (blen + kXzEncChunk - 1) / kXzEncChunk;
    xzenc_chains_host(blk, blen, prev, head);
    std::vector<XzEncWork> work(level ? 1 : 0);
    for (uint32_t k = 0; k < nch; ++k) {
        const uint32_t cs = k * kXzEncChunk, ce = std::min(blen, cs + kXzEncChunk);
        for (uint32_t i = 0; i < kXzEncProbs; ++i) probs[i] = (uint16_t)kLzmaProbInit;
        if (level) {
            for (uint32_t p = cs; p < ce; ++p) xzenc_find_set(blk, prev, p, ce, cand + (size_t)p * kXzEncCands);
            XzEncHostLanes ln{lanes_descending};
            res[k] = xzenc_chunk_priced(blk, cs, ce, cand, probs, work[0], slots + (size_t)k * kXzEncSlot, kXzEncSlot, ops, ln);
            continue;
        }
        for (uint32_t p = cs; p < ce; ++p) cand[p] = xzenc_find(blk, prev, p, ce);
        res[k] = xzenc_chunk(blk, cs, ce, cand, probs, slots + (size_t)k * kXzEncSlot, kXzEncSlot, ops);
    }
    return xzenc_block_layout(res, nch, blen, dst, check, filter);
}
// what lzma2_concat_kernel writes of a Block that begins at q: chunk headers, bodies and the end byte
inline void xzenc_block_place(const uint8_t* blk, uint32_t blen, const uint32_t* res, const uint64_t* dst, const uint8_t* slots, uint8_t* q)
{
    const uint32_t nch = (blen + kXzEncChunk - 1) / kXzEncChunk;
    for (uint32_t k = 0; k < nch; ++k) {
        const uint32_t cs = k * kXzEncChunk, usize = std::min(blen, cs + kXzEncChunk) - cs;
        const bool stored = res[k] == kXzEncStored;
        const uint32_t h = xzenc_chunk_header(q + dst[k], k == 0, usize, res[k]), len = stored ? usize : res[k];
        memcpy(q + dst[k] + h, stored ? blk + cs : slots + (size_t)k * kXzEncSlot, len);
        if (k + 1 == nch) q[dst[k] + h + len] = 0;
    }
}
// what the host writes of a Block that begins at q: header, Block Padding, Check (CRC-64, or any Check's field as bytes)
inline void xzenc_block_frame(uint8_t* q, const XzEncBlockLayout& L, uint64_t blen, uint32_t dict_byte, const uint8_t* field, uint32_t check_size,
                              const XzEncChain& filter = XzEncChain())
{
    xzenc_block_header(q, L.data, blen, dict_byte, filter);
    for (uint64_t z = L.hdr + L.data; z < L.check_at; ++z) q[z] = 0;
    if (check_size) memcpy(q + L.check_at, field, check_size);
}
inline void xzenc_block_frame(uint8_t* q, const XzEncBlockLayout& L, uint64_t blen, uint32_t dict_byte, uint64_t crc)
{
    uint8_t field[8];
    xzenc_le64(field, crc);
    xzenc_block_frame(q, L, blen, dict_byte, field, 8);
}

// The whole file on this thread, through the routines the kernels run, with Check `check` (xzenc_check_valid).
// field(p, len, out): the Check of a Block's bytes, xzenc_check_size(check) bytes as the file holds them.  false: the
// block size, the Check or the chain is not one the format decisions allow.  filter: the chain in front of LZMA2 (a plain id:
// one BCJ filter; 0: none): every Block is filtered as the kernels filter it (a copy, positions from the Block's first byte) and the steps run
// over the copy; the Check is over the unfiltered bytes.
template <class OPS, class FIELD>
inline bool xzenc_host(const uint8_t* data, uint64_t n, uint64_t block_size, uint32_t check, std::vector<uint8_t>& out, OPS& ops, FIELD field,
                       XzEncInfo* info = nullptr, const XzEncChain& filter = XzEncChain(), uint32_t level = 0, bool lanes_descending = false)
{
    if (!xzenc_block_size(&block_size) || !xzenc_check_valid(check) || !xzenc_chain_valid(filter) || level > kXzEncLevelMax) return false;
    const uint32_t dict_byte = xzenc_dict_byte(block_size), check_size = xzenc_check_size(check);
    out.resize(kXzEncStreamHeader);
    xzenc_stream_header(out.data(), check);
    std::vector<XzEncRecord> recs;
    std::vector<uint32_t> prev, cand, head(1u << kXzEncHashBits), res;
    std::vector<uint64_t> dst;
    std::vector<uint16_t> probs(kXzEncProbs);
    std::vector<uint8_t> slots, filtered;
    for (uint64_t b0 = 0; b0 < n; b0 += block_size) {
        const uint8_t* const raw = data + b0;
        const uint8_t* blk = raw;
        const uint32_t blen = (uint32_t)std::min<uint64_t>(block_size, n - b0);
        if (filter) {
            filtered.assign(raw, raw + blen);
            xzenc_chain_apply(filter, filtered.data(), blen);
            blk = filtered.data();
        }
        const uint32_t nch = (blen + kXzEncChunk - 1) / kXzEncChunk;
        prev.resize(blen);
        cand.resize((size_t)blen * (level ? kXzEncCands : 1));
        res.resize(nch);
        dst.resize(nch);
        slots.resize((size_t)nch * kXzEncSlot);
        const XzEncBlockLayout L = xzenc_block_stages(blk, blen, prev.data(), cand.data(), head.data(), probs.data(), res.data(), dst.data(),
                                                      slots.data(), ops, check, filter, level, lanes_descending);
        if (info)
            for (uint32_t k = 0; k < nch; ++k) {
                info->chunks++;
                info->stored += res[k] == kXzEncStored;
                info->res.push_back(res[k]);
            }
        const size_t o = out.size();
        out.resize(o + L.total, 0);
        uint8_t f[kXzEncCheckMax] = {0};
        field(raw, (uint64_t)blen, f);
        xzenc_block_frame(out.data() + o, L, blen, dict_byte, f, check_size, filter);
        xzenc_block_place(blk, blen, res.data(), dst.data(), slots.data(), out.data() + o);
        recs.push_back(XzEncRecord{L.unpadded, blen});
    }
    xzenc_index_footer(recs, out, check);
    return true;
}
// The same with the default Check.  crc64: the CRC-64 of a Block's bytes, as a number.
template <class OPS, class CRC>
inline bool xzenc_host(const uint8_t* data, uint64_t n, uint64_t block_size, std::vector<uint8_t>& out, OPS& ops, CRC crc64,
                       XzEncInfo* info = nullptr)
{
    return xzenc_host(data, n, block_size, (uint32_t)kXzCheckCrc64, out, ops, [&](const uint8_t* p, uint64_t len, uint8_t* f) { xzenc_le64(f, crc64(p, len)); },
                      info);
}

} // namespace snaphash
