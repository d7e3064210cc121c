// bz2enc_stage_model.h -- what snaphash_bzenc_stages_device's arrays must hold, from the host model's routines
// (snappy_amd/csrc/bzip2_enc_core.h), for tests/bz2enc_host_harness.cpp (be_stages, be_stages_from_last, be_read_slot) and
// the stand-alone sanitizer program tests/asan_bz2enc.cpp.  The caller hands every array in as the device buffers start
// out: slots, res and out zero (the launchers memset them), everything else the fill; what a stage does not write stays.
// Layout and strides are the producer's (snaphash.h states them).
#pragma once
#include <string.h>

#include "../snappy_amd/csrc/bzip2_enc_core.h"

namespace snaphash {

constexpr uint32_t kBeSelStride = 18048; // bzip2_enc_kernels.h's kBzEncSelStride (that header needs HIP's)
constexpr uint32_t kBeResWords = 6;      // BzEncRes: rle_n, orig_ptr, nmtf, bits, over, pad
constexpr uint8_t kBeFill = 0xA5;        // what the tests' buffers start out as
static_assert(sizeof(BzEncMap) == 516, "used[256], seq[256], nused");

struct BeArrays {
    uint8_t *rle, *last; // cap + 64 a block
    uint16_t* syms;      // cap + 64 a block
    uint8_t* maps;       // sizeof(BzEncMap) a block
    uint8_t* sel;        // kBeSelStride a block
    uint32_t* slots;     // bzenc_slot_words(cap) a block
    uint32_t* res;       // kBeResWords a block
    uint64_t* dst;
    uint32_t* out;
    uint64_t out_words;
    uint8_t* over;       // a flag a block: its RLE1 output exceeded cap (stages behind RLE1: don't care)
};

// RLE1 as the kernel stores it into a block's cap + 64 bytes: every source byte's emit (one byte, or the fourth byte of a
// group and its count) goes in whole while it ends at or before the room's end, else not at all.  Returns the length the
// output would have.
inline uint32_t be_rle1_capped(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t room)
{
    uint32_t o = 0, i = 0;
    while (i < n) {
        const uint8_t c = in[i];
        uint32_t run = 1;
        while (run < kBzEncRunMax && i + run < n && in[i + run] == c) ++run;
        for (uint32_t k = 0; k < run && k < 4; ++k) {
            const uint32_t e = k == 3 ? 2u : 1u;
            if (o + e <= room) {
                out[o] = c;
                if (e == 2) out[o + 1] = (uint8_t)(run - 4);
            }
            o += e;
        }
        i += run;
    }
    return o;
}

// MTF, coding and the slot of block k from its last column a.last[k][0 .. rn)
inline void be_block_from_last(const BeArrays& a, uint32_t k, uint32_t cap, uint32_t rn, uint32_t op, uint32_t crc)
{
    const uint32_t room = cap + 64, slot_words = bzenc_slot_words(cap);
    const uint8_t* last = a.last + (size_t)k * room;
    uint16_t* syms = a.syms + (size_t)k * room;
    uint8_t* sel = a.sel + (size_t)k * kBeSelStride;
    uint32_t* slot = a.slots + (size_t)k * slot_words;
    BzEncMap m;
    const uint32_t nmtf = bzenc_mtf(last, rn, m, syms); // (rn + 1 <= cap + 1 symbols at most)
    memcpy(a.maps + (size_t)k * sizeof(BzEncMap), &m, sizeof m);
    std::vector<BzEncHuff> hh(1);
    BzEncHuffScratch s;
    const uint32_t ng = bzenc_groups(nmtf);
    const uint32_t nt = bzenc_huffman(hh[0], s, m.nused + 2, syms, nmtf, sel);
    BzW w;
    bzw_start(w, slot, slot_words, 0);
    bzenc_write_head(w, crc, op, m, hh[0], nt, sel, ng);
    for (uint32_t g = 0; g < ng; ++g) {
        const uint32_t g0 = g * kBzEncGroup, cnt = std::min(kBzEncGroup, nmtf - g0);
        bzenc_write_group(w, hh[0], sel[g], syms + g0, cnt);
    }
    const uint64_t bits = bzw_pos(w);
    bzw_flush(w);
    uint32_t* r = a.res + (size_t)k * kBeResWords;
    r[0] = rn; r[1] = op; r[2] = nmtf; r[3] = (uint32_t)bits; r[4] = w.over; r[5] = 0;
}

// The host's placement and the concat kernel: returns the bit behind the last block, or -1 when a block is over (dst and
// out are then not written); out_words too small: the total all the same, dst and out not written.
inline int64_t be_place_and_concat(const BeArrays& a, uint32_t nblk, uint32_t cap, uint32_t carry, uint32_t carry_bits)
{
    const uint32_t slot_words = bzenc_slot_words(cap);
    for (uint32_t k = 0; k < nblk; ++k)
        if (a.over[k] || a.res[(size_t)k * kBeResWords + 4]) return -1;
    uint64_t at = carry_bits;
    std::vector<uint64_t> dst(nblk);
    for (uint32_t k = 0; k < nblk; ++k) {
        dst[k] = at;
        at += a.res[(size_t)k * kBeResWords + 3];
    }
    if ((at + 31) / 32 > a.out_words) return (int64_t)at;
    for (uint64_t i = 0; i < a.out_words; ++i) a.out[i] = 0;
    a.out[0] |= carry & 0xffu; // (memory in stream order: byte 0)
    for (uint32_t k = 0; k < nblk; ++k) {
        a.dst[k] = dst[k];
        const uint32_t* slot = a.slots + (size_t)k * slot_words;
        const uint32_t bits = a.res[(size_t)k * kBeResWords + 3];
        BzW w;
        bzw_start(w, a.out, (uint32_t)a.out_words, dst[k]);
        uint32_t j = 0;
        for (; j < bits / 32; ++j) bzw_put(w, bzenc_bswap(slot[j]), 32);
        if (bits & 31) bzw_put(w, bzenc_bswap(slot[j]) >> (32 - (bits & 31)), bits & 31);
        bzw_flush(w);
    }
    return (int64_t)at;
}

// Every array for nblk ranges of data (each 1 .. bzenc_piece(level) bytes), cap a multiple of 64.
inline int64_t be_stages_host(const uint8_t* data, const uint64_t* offs, const uint64_t* lens, uint32_t nblk, uint32_t cap, uint32_t carry,
                              uint32_t carry_bits, const BeArrays& a)
{
    static const struct Tab { uint32_t t[256]; Tab() { bz_crc_table(t); } } tab;
    const uint32_t room = cap + 64;
    for (uint32_t k = 0; k < nblk; ++k) {
        const uint8_t* piece = data + offs[k];
        const uint32_t n = (uint32_t)lens[k];
        const uint32_t crc = ~bz_crc_update(tab.t, ~0u, piece, n);
        uint8_t* rle = a.rle + (size_t)k * room;
        const uint32_t rn = be_rle1_capped(piece, n, rle, room);
        a.over[k] = rn > cap;
        if (rn > cap) { // rle_n 0, over 1; what MTF and coding make of an empty block is not stated
            a.res[(size_t)k * kBeResWords + 0] = 0;
            a.res[(size_t)k * kBeResWords + 4] = 1;
            continue;
        }
        const uint32_t op = bzenc_bwt_host(rle, rn, a.last + (size_t)k * room);
        be_block_from_last(a, k, cap, rn, op, crc);
    }
    return be_place_and_concat(a, nblk, cap, carry, carry_bits);
}

// The same from last columns the caller has put into a.last (block k: rle_n[k] bytes, 1 .. cap).
inline int64_t be_stages_from_last_host(const uint32_t* rle_n, const uint32_t* orig_ptr, const uint32_t* crc, uint32_t nblk, uint32_t cap,
                                        uint32_t carry, uint32_t carry_bits, const BeArrays& a)
{
    for (uint32_t k = 0; k < nblk; ++k) {
        a.over[k] = 0;
        be_block_from_last(a, k, cap, rle_n[k], orig_ptr[k], crc[k]);
    }
    return be_place_and_concat(a, nblk, cap, carry, carry_bits);
}

// One slot's bits taken back by the install side's decoder (bzip2_core.h bz_block_symbols): the last column into
// last[0 .. cap_out), its length, origPtr and the stored CRC, the bit the block ended at.  Returns the decoder's status.
inline int32_t be_read_slot_host(const uint32_t* slot, uint32_t slot_words, uint8_t* last, uint32_t cap_out, uint32_t* n, uint32_t* op, uint32_t* crc,
                                 uint64_t* end_bit)
{
    std::vector<BzTables> tt(1);
    const BzBlockRes r = bz_block_symbols((const uint8_t*)slot, (uint64_t)slot_words * 4, 0, last, cap_out, nullptr, tt[0]);
    *n = r.n;
    *op = r.orig_ptr;
    *crc = r.crc;
    *end_bit = r.end_bit;
    return r.status;
}

} // namespace snaphash
