// bzip2_enc_core.h -- the bzip2 encoder of the data.tar.bz2 producer (bzpack.inc), shared by the GPU kernels
// (bzip2_enc_kernels.hip), the host model in tests/bz2enc_host_harness.cpp and the stand-alone sanitizer program, the way
// xz_enc_core.h serves the .xz side.  DESIGN.md sec. 21.
//
// The stream is "BZh" + the level digit, one block per PIECE of input, the end-of-stream magic, the combined CRC and
// padding to a byte.  Pieces are cut by input size, bzenc_piece(level) bytes each, so that blocks are independent before a
// byte is coded: RLE1 expands by 5/4 at most (a run of exactly four becomes five bytes), and 5/4 of a piece never exceeds
// libbz2's own 100 000 x level - 19.  A run cut by a piece's end is two runs.
//
// Stages of one block, each a plain function here (the host model) and a kernel that gives the same bytes:
//   bzenc_rle1        runs of 4..259 equal bytes become four bytes and a count
//   bzenc_bwt_host    the last column of the sorted cyclic rotations and origPtr (the kernel sorts by prefix doubling with
//                     radix passes; the model sorts packed keys: L and origPtr are defined by the order, not the algorithm;
//                     equal rotations -- a block periodic after RLE1 -- are ordered by start index)
//   bzenc_mtf         the used-byte map, move-to-front, RUNA/RUNB zero-run coding, EOB
//   bzenc_huffman     libbz2's scheme: 2-6 tables by nMTF, the initial partition by cumulative frequency, four refinement
//                     rounds over groups of 50 (cheapest table, lowest index on a tie), code lengths limited to 17 bits
//   bzenc_write_head  the block header, the selectors (MTF, unary), the tables (delta coded from a 5-bit start)
//   bzenc_write_group one group of 50 symbols, MSB first
// Every decision is integer arithmetic with a stated tie rule, so kernel and model agree byte for byte.
#pragma once
#include <stdint.h>

#include "bzip2_core.h"

#if !defined(__HIP_DEVICE_COMPILE__)
#include <algorithm>
#include <vector>
#endif

namespace snaphash {

constexpr uint32_t kBzEncGroup = 50;      // symbols a selector covers (libbz2's BZ_G_SIZE)
constexpr uint32_t kBzEncMaxBits = 17;    // longest code written (libbz2 writes 17; decoders take 20)
constexpr uint32_t kBzEncRounds = 4;      // refinement rounds (libbz2's BZ_N_ITERS)
constexpr uint32_t kBzEncAlphaMax = 258;  // RUNA, RUNB, 255 MTF positions, EOB
constexpr uint32_t kBzEncRunMax = 259;    // source bytes of one RLE1 group: four and a count of up to 255
constexpr uint32_t kBzEncStreamHead = 4, kBzEncStreamTail = 10;

// 1..9, 0 for the default (9); 0 returned for anything else
BZ_HD uint32_t bzenc_level(uint32_t level) { return level == 0 ? 9u : (level <= 9 ? level : 0u); }
// input bytes of a block: 719 872 at level 9, 79 872 at level 1 (a multiple of the tar record)
BZ_HD uint32_t bzenc_piece(uint32_t level) { return (100000u * level - 19u) * 4u / 5u / 512u * 512u; }
// what a piece is after RLE1, at most (<= 100 000 x level - 19)
BZ_HD uint32_t bzenc_rle_cap(uint32_t level) { return bzenc_piece(level) / 4u * 5u; }
BZ_HD uint32_t bzenc_groups(uint32_t nmtf) { return (nmtf + kBzEncGroup - 1) / kBzEncGroup; }
// 32-bit words of a block's output slot for n BWT bytes: 17 bits a symbol (n + 1 with EOB; a zero run codes to no more
// symbols than it has bytes) and the header's worst case -- magic, CRC, randomised bit, origPtr, the symbol map, the table
// and selector counts, kBzMaxSelectors selectors of up to 6 bits, six tables of a 5-bit start and 258 lengths at up to
// 16 two-bit moves and a stop bit each
BZ_HD uint32_t bzenc_slot_words(uint32_t n)
{
    const uint64_t bits = 48 + 32 + 1 + 24 + 16 + 256 + 3 + 15 + (uint64_t)kBzMaxSelectors * 6 + 6 * (5 + 258 * 33) + (uint64_t)kBzEncMaxBits * (n + 1);
    return (uint32_t)((bits + 31) / 32 + 2);
}

// ---- bits, MSB first ----
// A writer ORs whole 32-bit words (stored so that memory is in stream order) into a zeroed buffer from any bit offset,
// so writers of neighbouring ranges may share a word: on the device the OR is atomic.  Words at or past `cap` are dropped
// (and `over` set): by bzenc_slot_words none is.
struct BzW {
    uint32_t* out;
    uint32_t cap; // words
    uint32_t wi;  // next word
    uint32_t cnt; // bits in acc (< 32 between calls)
    uint64_t acc; // left-aligned
    uint32_t over;
};
BZ_HD uint32_t bzenc_bswap(uint32_t v) { return v >> 24 | (v >> 8 & 0xff00u) | (v << 8 & 0xff0000u) | v << 24; }
BZ_HD void bzw_start(BzW& w, uint32_t* out, uint32_t cap_words, uint64_t bit)
{
    w.out = out;
    w.cap = cap_words;
    w.wi = (uint32_t)(bit >> 5);
    w.cnt = (uint32_t)(bit & 31);
    w.acc = 0;
    w.over = 0;
}
BZ_HD void bzw_word(BzW& w, uint32_t v)
{
    if (w.wi < w.cap) {
        if (v) {
#if defined(__HIP_DEVICE_COMPILE__)
            atomicOr(&w.out[w.wi], bzenc_bswap(v));
#else
            w.out[w.wi] |= bzenc_bswap(v);
#endif
        }
    } else {
        w.over = 1;
    }
    ++w.wi;
}
BZ_HD void bzw_put(BzW& w, uint32_t v, uint32_t n) // 1 <= n <= 32, v < 2^n
{
    w.acc |= (uint64_t)v << (64 - w.cnt - n);
    w.cnt += n;
    if (w.cnt >= 32) {
        bzw_word(w, (uint32_t)(w.acc >> 32));
        w.acc <<= 32;
        w.cnt -= 32;
    }
}
BZ_HD uint64_t bzw_pos(const BzW& w) { return (uint64_t)w.wi * 32 + w.cnt; }
BZ_HD void bzw_flush(BzW& w)
{
    if (w.cnt) bzw_word(w, (uint32_t)(w.acc >> 32));
    w.cnt = 0;
    w.acc = 0;
}

// ---- RLE1 ----
// What source byte i of a piece emits: of each group of up to 259 equal bytes the first four emit themselves and the
// fourth also the count of those that follow it in the group (0..255).  p: i's place in its run of equal bytes.
BZ_HD uint32_t bzenc_rle1_emits(uint32_t p)
{
    const uint32_t q = p % kBzEncRunMax;
    return q < 3 ? 1u : (q == 3 ? 2u : 0u);
}
// in[0..n) -> out (room for n / 4 * 5 + 4 bytes); returns the length
BZ_HD uint32_t bzenc_rle1(const uint8_t* in, uint32_t n, uint8_t* out)
{
    uint32_t o = 0, i = 0;
    while (i < n) {
        const uint8_t c = in[i];
        uint32_t run = 1;
        while (run < kBzEncRunMax && i + run < n && in[i + run] == c) ++run;
        for (uint32_t k = 0; k < run && k < 4; ++k) out[o++] = c;
        if (run >= 4) out[o++] = (uint8_t)(run - 4);
        i += run;
    }
    return o;
}

// ---- BWT (the model) ----
#if !defined(__HIP_DEVICE_COMPILE__)
// The first key of rotation i: its first four bytes (cyclic).  The kernel starts from the same key.
inline uint32_t bzenc_key4(const uint8_t* b, uint32_t n, uint32_t i)
{
    uint32_t k = 0;
    for (uint32_t j = 0; j < 4; ++j) k = k << 8 | b[(i + j) % n];
    return k;
}
// last[j] = b[(sa[j] + n - 1) % n] over the sorted cyclic rotations of b[0..n), 1 <= n < 2^20; returns origPtr, the
// number of rotations that sort before rotation 0 (equal rotations by start index).
inline uint32_t bzenc_bwt_host(const uint8_t* b, uint32_t n, uint8_t* last)
{
    std::vector<uint64_t> key(n);
    std::vector<uint32_t> rank(n);
    for (uint32_t i = 0; i < n; ++i) key[i] = (uint64_t)bzenc_key4(b, n, i) << 20 | i;
    for (uint64_t k = 4;; k *= 2) {
        std::sort(key.begin(), key.end()); // (the start index in the low bits: ties by start index)
        uint32_t r = 0;
        for (uint32_t j = 0; j < n; ++j) {
            if (j && (key[j] >> 20) != (key[j - 1] >> 20)) ++r;
            rank[(uint32_t)(key[j] & 0xfffffu)] = r;
        }
        if (r == n - 1 || k >= n) break;
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t i = (uint32_t)(key[j] & 0xfffffu);
            key[j] = ((uint64_t)rank[i] << 20 | rank[(uint32_t)((i + k) % n)]) << 20 | i;
        }
    }
    uint32_t op = 0;
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t i = (uint32_t)(key[j] & 0xfffffu);
        if (i == 0) op = j;
        last[j] = b[i ? i - 1 : n - 1];
    }
    return op;
}
#endif

// ---- MTF, zero runs, the symbol map ----
struct BzEncMap {
    uint8_t used[256]; // 1: the byte occurs in the block
    uint8_t seq[256];  // byte value -> its index among the used ones
    uint32_t nused;
};
BZ_HD void bzenc_map_finish(BzEncMap& m) // used[] -> seq[], nused
{
    uint32_t k = 0;
    for (uint32_t c = 0; c < 256; ++c) {
        m.seq[c] = (uint8_t)k;
        k += m.used[c] ? 1u : 0u;
    }
    m.nused = k;
}
// a run of `run` >= 1 front bytes as RUNA (0) / RUNB (1), bijective base 2, least digit first, through store(at, symbol);
// returns the new count.  The kernel's wave calls it with a store that only lane 0 performs, inside its buffer.
template <class Store> BZ_HD uint32_t bzenc_put_run_to(Store&& store, uint32_t w, uint32_t run)
{
    --run;
    for (;;) {
        store(w++, (uint16_t)(run & 1u));
        if (run < 2) break;
        run = (run - 2) / 2;
    }
    return w;
}
BZ_HD uint32_t bzenc_put_run(uint16_t* syms, uint32_t w, uint32_t run)
{
    return bzenc_put_run_to([syms](uint32_t at, uint16_t v) { syms[at] = v; }, w, run);
}
// last[0..n) -> syms (room for n + 1), the map; returns nMTF (EOB included)
BZ_HD uint32_t bzenc_mtf(const uint8_t* last, uint32_t n, BzEncMap& m, uint16_t* syms)
{
    for (uint32_t c = 0; c < 256; ++c) m.used[c] = 0;
    for (uint32_t i = 0; i < n; ++i) m.used[last[i]] = 1;
    bzenc_map_finish(m);
    uint8_t yy[256];
    for (uint32_t i = 0; i < 256; ++i) yy[i] = (uint8_t)i;
    uint32_t w = 0, run = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t v = m.seq[last[i]];
        if (yy[0] == v) {
            ++run;
            continue;
        }
        if (run) w = bzenc_put_run(syms, w, run);
        run = 0;
        uint32_t p = 1;
        while (yy[p] != v) ++p;
        for (uint32_t k = p; k > 0; --k) yy[k] = yy[k - 1];
        yy[0] = v;
        syms[w++] = (uint16_t)(p + 1);
    }
    if (run) w = bzenc_put_run(syms, w, run);
    syms[w++] = (uint16_t)(m.nused + 1); // EOB
    return w;
}

// ---- Huffman ----
BZ_HD uint32_t bzenc_ntables(uint32_t nmtf) { return nmtf < 200 ? 2u : nmtf < 600 ? 3u : nmtf < 1200 ? 4u : nmtf < 2400 ? 5u : 6u; }

struct BzEncHuff {
    uint8_t len[6][kBzEncAlphaMax];
    uint32_t code[6][kBzEncAlphaMax];
    uint32_t rfreq[6][kBzEncAlphaMax];
    uint32_t freq[kBzEncAlphaMax];
};
struct BzEncHuffScratch {
    uint32_t w[2 * kBzEncAlphaMax];
    uint32_t f[kBzEncAlphaMax];
    uint16_t parent[2 * kBzEncAlphaMax];
    uint16_t order[kBzEncAlphaMax];
};

// libbz2's initial partition: table nPart-1 is cheap (0) for a run of symbols of about 1/nPart of what is left, dear (15)
// for the rest
BZ_HD void bzenc_initial_lens(BzEncHuff& h, uint32_t alpha, uint32_t nt, uint32_t nmtf)
{
    int32_t gs = 0;
    uint32_t rem = nmtf;
    for (uint32_t part = nt; part > 0; --part) {
        const uint32_t target = rem / part;
        int32_t ge = gs - 1;
        uint32_t a = 0;
        while (a < target && ge < (int32_t)alpha - 1) {
            ++ge;
            a += h.freq[ge];
        }
        if (ge > gs && part != nt && part != 1 && ((nt - part) % 2 == 1)) {
            a -= h.freq[ge];
            --ge;
        }
        for (int32_t v = 0; v < (int32_t)alpha; ++v) h.len[part - 1][v] = (v >= gs && v <= ge) ? 0 : 15;
        gs = ge + 1;
        rem -= a;
    }
}

// the table that codes syms[0..cnt) in the fewest bits; the lowest index wins a tie
BZ_HD uint32_t bzenc_pick_table(const BzEncHuff& h, uint32_t nt, const uint16_t* syms, uint32_t cnt)
{
    uint32_t cost[6] = {0, 0, 0, 0, 0, 0};
    for (uint32_t i = 0; i < cnt; ++i) {
        const uint32_t s = syms[i];
        for (uint32_t t = 0; t < nt; ++t) cost[t] += h.len[t][s];
    }
    uint32_t best = 0;
    for (uint32_t t = 1; t < nt; ++t)
        if (cost[t] < cost[best]) best = t;
    return best;
}

// Code lengths 1..max_bits for alpha symbols, every one coded (a frequency of 0 counts as 1, as in libbz2).  A twin of
// deflate_core.h's huff_lengths, which clamps frequencies to 16 bits -- a block here has up to 900 000 symbols.  Symbols
// sorted by (weight, index); two-queue merge, a tie between a leaf and an internal node goes to the leaf; a tree deeper
// than max_bits is built again from weights 1 + w / 2 (libbz2's rule), at most 32 times: then all are 1.
BZ_HD void bzenc_code_lengths(const uint32_t* freq, uint32_t alpha, uint32_t max_bits, uint8_t* len, BzEncHuffScratch& s)
{
    const int n = (int)alpha;
    for (int i = 0; i < n; ++i) s.f[i] = freq[i] ? freq[i] : 1u;
    for (uint32_t round = 0; round < 33; ++round) {
        for (int i = 0; i < n; ++i) { // insertion sort by (weight, index)
            const uint32_t fi = s.f[i];
            int j = i;
            while (j > 0 && s.f[s.order[j - 1]] > fi) {
                s.order[j] = s.order[j - 1];
                --j;
            }
            s.order[j] = (uint16_t)i;
        }
        for (int i = 0; i < n; ++i) s.w[i] = s.f[s.order[i]];
        int li = 0, ii = n, nn = n;
        for (int k = 0; k < n - 1; ++k) {
            int a, b;
            if (li < n && (ii >= nn || s.w[li] <= s.w[ii])) a = li++; else a = ii++;
            if (li < n && (ii >= nn || s.w[li] <= s.w[ii])) b = li++; else b = ii++;
            s.w[nn] = s.w[a] + s.w[b];
            s.parent[a] = (uint16_t)nn;
            s.parent[b] = (uint16_t)nn;
            ++nn;
        }
        s.w[nn - 1] = 0;
        uint32_t deepest = 0;
        for (int node = nn - 2; node >= 0; --node) {
            s.w[node] = s.w[s.parent[node]] + 1u;
            if (node < n && s.w[node] > deepest) deepest = s.w[node];
        }
        if (deepest <= max_bits) {
            for (int i = 0; i < n; ++i) len[s.order[i]] = (uint8_t)s.w[i];
            return;
        }
        for (int i = 0; i < n; ++i) s.f[i] = 1u + s.f[i] / 2u;
    }
}

// canonical codes: by length, then by symbol
BZ_HD void bzenc_assign_codes(const uint8_t* len, uint32_t alpha, uint32_t* code)
{
    uint32_t v = 0;
    for (uint32_t l = 1; l <= 20; ++l) {
        for (uint32_t i = 0; i < alpha; ++i)
            if (len[i] == l) code[i] = v++;
        v <<= 1;
    }
}

// One refinement round's first half over groups [g0, g1): selectors and the tables' new frequencies (h.rfreq zeroed by
// the caller).  The kernel runs the same two calls per group with an atomic add.
BZ_HD void bzenc_assign_groups(BzEncHuff& h, uint32_t nt, const uint16_t* syms, uint32_t nmtf, uint8_t* sel)
{
    const uint32_t ng = bzenc_groups(nmtf);
    for (uint32_t g = 0; g < ng; ++g) {
        const uint32_t g0 = g * kBzEncGroup, cnt = nmtf - g0 < kBzEncGroup ? nmtf - g0 : kBzEncGroup;
        const uint32_t t = bzenc_pick_table(h, nt, syms + g0, cnt);
        sel[g] = (uint8_t)t;
        for (uint32_t i = 0; i < cnt; ++i) h.rfreq[t][syms[g0 + i]]++;
    }
}

// all of it, serially: returns the table count; sel[groups], h.len / h.code filled
BZ_HD uint32_t bzenc_huffman(BzEncHuff& h, BzEncHuffScratch& s, uint32_t alpha, const uint16_t* syms, uint32_t nmtf, uint8_t* sel)
{
    for (uint32_t i = 0; i < alpha; ++i) h.freq[i] = 0;
    for (uint32_t i = 0; i < nmtf; ++i) h.freq[syms[i]]++;
    const uint32_t nt = bzenc_ntables(nmtf);
    bzenc_initial_lens(h, alpha, nt, nmtf);
    for (uint32_t r = 0; r < kBzEncRounds; ++r) {
        for (uint32_t t = 0; t < nt; ++t)
            for (uint32_t i = 0; i < alpha; ++i) h.rfreq[t][i] = 0;
        bzenc_assign_groups(h, nt, syms, nmtf, sel);
        for (uint32_t t = 0; t < nt; ++t) bzenc_code_lengths(h.rfreq[t], alpha, kBzEncMaxBits, h.len[t], s);
    }
    for (uint32_t t = 0; t < nt; ++t) bzenc_assign_codes(h.len[t], alpha, h.code[t]);
    return nt;
}

// the block's header at w (the block's first bit): returns nothing; the symbols follow at bzw_pos(w)
BZ_HD void bzenc_write_head(BzW& w, uint32_t crc, uint32_t orig_ptr, const BzEncMap& m, const BzEncHuff& h, uint32_t nt, const uint8_t* sel,
                            uint32_t nsel)
{
    bzw_put(w, (uint32_t)(kBzBlockMagic >> 24), 24);
    bzw_put(w, (uint32_t)(kBzBlockMagic & 0xffffffu), 24);
    bzw_put(w, crc, 32);
    bzw_put(w, 0, 1); // not randomised
    bzw_put(w, orig_ptr, 24);
    uint32_t rows = 0;
    for (uint32_t i = 0; i < 16; ++i)
        for (uint32_t j = 0; j < 16; ++j)
            if (m.used[i * 16 + j]) rows |= 0x8000u >> i;
    bzw_put(w, rows, 16);
    for (uint32_t i = 0; i < 16; ++i) {
        if (!(rows & (0x8000u >> i))) continue;
        uint32_t row = 0;
        for (uint32_t j = 0; j < 16; ++j)
            if (m.used[i * 16 + j]) row |= 0x8000u >> j;
        bzw_put(w, row, 16);
    }
    bzw_put(w, nt, 3);
    bzw_put(w, nsel, 15);
    uint8_t pos[6] = {0, 1, 2, 3, 4, 5};
    for (uint32_t i = 0; i < nsel; ++i) {
        const uint8_t v = sel[i];
        uint32_t j = 0;
        while (pos[j] != v) ++j;
        for (uint32_t k = j; k > 0; --k) pos[k] = pos[k - 1];
        pos[0] = v;
        bzw_put(w, (1u << (j + 1)) - 2u, j + 1); // j ones and a zero
    }
    const uint32_t alpha = m.nused + 2;
    for (uint32_t t = 0; t < nt; ++t) {
        uint32_t cur = h.len[t][0];
        bzw_put(w, cur, 5);
        for (uint32_t i = 0; i < alpha; ++i) {
            while (cur < h.len[t][i]) { bzw_put(w, 2, 2); ++cur; }
            while (cur > h.len[t][i]) { bzw_put(w, 3, 2); --cur; }
            bzw_put(w, 0, 1);
        }
    }
}

BZ_HD uint32_t bzenc_group_bits(const BzEncHuff& h, uint32_t t, const uint16_t* syms, uint32_t cnt)
{
    uint32_t b = 0;
    for (uint32_t i = 0; i < cnt; ++i) b += h.len[t][syms[i]];
    return b;
}
BZ_HD void bzenc_write_group(BzW& w, const BzEncHuff& h, uint32_t t, const uint16_t* syms, uint32_t cnt)
{
    for (uint32_t i = 0; i < cnt; ++i) bzw_put(w, h.code[t][syms[i]], h.len[t][syms[i]]);
}

// ---- the whole stream (the model) ----
#if !defined(__HIP_DEVICE_COMPILE__)
struct BzEncBlockInfo { // what the model's stages gave, for the tests
    uint32_t rle_n, orig_ptr, nmtf, ntables, nsel, crc;
    uint64_t bits;
};

// One block of piece[0..n), n >= 1, appended to the stream at bit `at` of `out` (words, zero beyond); returns the new bit.
inline uint64_t bzenc_block_host(const uint8_t* piece, uint32_t n, std::vector<uint32_t>& out, uint64_t at, BzEncBlockInfo* info)
{
    static const struct Tab { uint32_t t[256]; Tab() { bz_crc_table(t); } } tab;
    const uint32_t crc = ~bz_crc_update(tab.t, ~0u, piece, n);
    std::vector<uint8_t> rle((size_t)n / 4 * 5 + 8), last;
    const uint32_t rn = bzenc_rle1(piece, n, rle.data());
    last.resize(rn);
    const uint32_t op = bzenc_bwt_host(rle.data(), rn, last.data());
    std::vector<uint16_t> syms((size_t)rn + 1);
    BzEncMap m;
    const uint32_t nmtf = bzenc_mtf(last.data(), rn, m, syms.data());
    std::vector<uint8_t> sel(bzenc_groups(nmtf));
    std::vector<BzEncHuff> hh(1);
    BzEncHuff& h = hh[0];
    BzEncHuffScratch s;
    const uint32_t nt = bzenc_huffman(h, s, m.nused + 2, syms.data(), nmtf, sel.data());
    out.resize((size_t)(at / 32) + bzenc_slot_words(rn) + 2, 0u);
    BzW w;
    bzw_start(w, out.data(), (uint32_t)out.size(), at);
    bzenc_write_head(w, crc, op, m, h, nt, sel.data(), (uint32_t)sel.size());
    for (uint32_t g = 0; g < sel.size(); ++g) {
        const uint32_t g0 = g * kBzEncGroup, cnt = std::min(kBzEncGroup, nmtf - g0);
        bzenc_write_group(w, h, sel[g], syms.data() + g0, cnt);
    }
    const uint64_t end = bzw_pos(w);
    bzw_flush(w);
    if (info) *info = BzEncBlockInfo{rn, op, nmtf, nt, (uint32_t)sel.size(), crc, end - at};
    return end;
}

// the footer behind the last block at bit `at`: returns the stream's length in bytes
inline uint64_t bzenc_footer_host(std::vector<uint32_t>& out, uint64_t at, uint32_t combined)
{
    out.resize((size_t)(at / 32) + 4, 0u);
    BzW w;
    bzw_start(w, out.data(), (uint32_t)out.size(), at);
    bzw_put(w, (uint32_t)(kBzEosMagic >> 24), 24);
    bzw_put(w, (uint32_t)(kBzEosMagic & 0xffffffu), 24);
    bzw_put(w, combined, 32);
    const uint64_t end = bzw_pos(w);
    bzw_flush(w);
    return (end + 7) / 8;
}

// data[0..n) at `level` (1..9) -> the .bz2 stream
inline std::vector<uint8_t> bzenc_stream_host(const uint8_t* data, uint64_t n, uint32_t level, std::vector<BzEncBlockInfo>* infos = nullptr)
{
    std::vector<uint32_t> out(1, 0u);
    BzW w;
    bzw_start(w, out.data(), 1, 0);
    bzw_put(w, 0x425a6830u + level, 32); // "BZh" + the digit
    uint64_t at = 32;
    uint32_t combined = 0;
    const uint32_t P = bzenc_piece(level);
    for (uint64_t off = 0; off < n; off += P) {
        BzEncBlockInfo bi;
        at = bzenc_block_host(data + off, (uint32_t)std::min<uint64_t>(P, n - off), out, at, &bi);
        combined = bz_crc_combine(combined, bi.crc);
        if (infos) infos->push_back(bi);
    }
    const uint64_t bytes = bzenc_footer_host(out, at, combined);
    std::vector<uint8_t> z((size_t)bytes);
    for (uint64_t i = 0; i < bytes; ++i) z[i] = (uint8_t)(out[i / 4] >> (8 * (i % 4))); // (words are stored in stream order)
    return z;
}
#endif

} // namespace snaphash
