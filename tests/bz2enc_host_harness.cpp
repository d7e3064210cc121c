// bz2enc_host_harness.cpp -- the .bz2 writer's host model (snappy_amd/csrc/bzip2_enc_core.h: the routines the GPU kernels
// run, stage by stage) compiled for the host, for tests/test_bz2enc_host.py and as the expected bytes of
// tests/test_gpu_bz2enc.py; a reader of what it wrote, built on bzip2_core.h's bit reader and block decoder; and every array
// the kernels leave, stage by stage (bz2enc_stage_model.h), as the expected arrays of tests/test_gpu_bz2enc_edges.py.
#include <stdlib.h>
#include <string.h>

#include "../snappy_amd/csrc/bzip2_enc_core.h"
#include "bz2enc_stage_model.h"

using namespace snaphash;

extern "C" {

constexpr size_t kInfoWords = 8; // per block: rle_n, orig_ptr, nmtf, ntables, nsel, crc, bits, 0

// the stream of data[0..n) at `level` (1..9); infos: kInfoWords uint64 a block, up to info_cap blocks; *blocks: how many
void* be_encode(const uint8_t* data, size_t n, uint32_t level, size_t* len, uint64_t* infos, size_t info_cap, size_t* blocks)
{
    std::vector<BzEncBlockInfo> bi;
    const std::vector<uint8_t> z = bzenc_stream_host(data, n, level, &bi);
    for (size_t k = 0; k < bi.size() && k < info_cap; ++k) {
        uint64_t* o = infos + k * kInfoWords;
        o[0] = bi[k].rle_n; o[1] = bi[k].orig_ptr; o[2] = bi[k].nmtf; o[3] = bi[k].ntables; o[4] = bi[k].nsel; o[5] = bi[k].crc; o[6] = bi[k].bits; o[7] = 0;
    }
    if (blocks) *blocks = bi.size();
    void* p = malloc(z.size() ? z.size() : 1);
    memcpy(p, z.data(), z.size());
    *len = z.size();
    return p;
}
void be_free(void* p) { free(p); }

uint32_t be_piece(uint32_t level) { return bzenc_piece(level); }
uint32_t be_ntables(uint32_t nmtf) { return bzenc_ntables(nmtf); }

// RLE1 of in[0..n) into out (room for n / 4 * 5 + 8); returns the length
uint32_t be_rle1(const uint8_t* in, uint32_t n, uint8_t* out) { return bzenc_rle1(in, n, out); }

// the BWT stage: last column into last[0..n), returns origPtr
uint32_t be_bwt(const uint8_t* in, uint32_t n, uint8_t* last) { return bzenc_bwt_host(in, n, last); }

// MTF + zero runs of last[0..n): symbols into syms (room for n + 1), returns nMTF; *nused: the used bytes
uint32_t be_mtf(const uint8_t* last, uint32_t n, uint16_t* syms, uint32_t* nused)
{
    BzEncMap m;
    const uint32_t w = bzenc_mtf(last, n, m, syms);
    *nused = m.nused;
    return w;
}

// code lengths of `alpha` symbols from freq, at most max_bits
void be_code_lengths(const uint32_t* freq, uint32_t alpha, uint32_t max_bits, uint8_t* len)
{
    BzEncHuffScratch s;
    bzenc_code_lengths(freq, alpha, max_bits, len, s);
}

uint32_t be_slot_words(uint32_t cap) { return bzenc_slot_words(cap); }
uint32_t be_rle_cap(uint32_t level) { return (bzenc_rle_cap(level) + 63) & ~63u; } // what the producer gives a fresh ctx

// What snaphash_bzenc_stages_device must leave in every array (bz2enc_stage_model.h): nblk ranges of data, cap a multiple of
// 64.  The caller hands the arrays in as the device buffers start out (slots, res, out zero; the rest the fill).  Returns
// the bit behind the last block; -1 when a block's RLE1 output exceeds cap (over[k] says which; dst and out as they were).
int64_t be_stages(const uint8_t* data, const uint64_t* offs, const uint64_t* lens, uint32_t nblk, uint32_t cap, uint32_t carry, uint32_t carry_bits,
                  uint8_t* rle, uint8_t* last, uint16_t* syms, uint8_t* maps, uint8_t* sel, uint32_t* slots, uint32_t* res, uint64_t* dst, uint32_t* out,
                  uint64_t out_words, uint8_t* over)
{
    const BeArrays a = {rle, last, syms, maps, sel, slots, res, dst, out, out_words, over};
    return be_stages_host(data, offs, lens, nblk, cap, carry, carry_bits, a);
}
// the same behind the BWT: block k's last column is last[k * (cap + 64) ..][0 .. rle_n[k])
int64_t be_stages_from_last(const uint32_t* rle_n, const uint32_t* orig_ptr, const uint32_t* crc, uint32_t nblk, uint32_t cap, uint32_t carry,
                            uint32_t carry_bits, uint8_t* last, uint16_t* syms, uint8_t* maps, uint8_t* sel, uint32_t* slots, uint32_t* res,
                            uint64_t* dst, uint32_t* out, uint64_t out_words, uint8_t* over)
{
    const BeArrays a = {nullptr, last, syms, maps, sel, slots, res, dst, out, out_words, over};
    return be_stages_from_last_host(rle_n, orig_ptr, crc, nblk, cap, carry, carry_bits, a);
}
// one slot's bits back to the last column, origPtr and CRC by the install side's decoder; returns its status (0: a whole block)
int32_t be_read_slot(const uint32_t* slot, uint32_t slot_words, uint8_t* last, uint32_t cap_out, uint32_t* n, uint32_t* op, uint32_t* crc,
                     uint64_t* end_bit)
{
    return be_read_slot_host(slot, slot_words, last, cap_out, n, op, crc, end_bit);
}

// Reads a stream this side wrote: per block (8 uint64): the bit it starts at, its CRC, origPtr, the table count, the
// selector count, the longest code length of any table, the BWT bytes it decodes to, the used-byte count.  Returns the
// block count, -1 for a stream that does not parse; *level, *combined (the stored one), *folded (from the blocks).
int64_t be_parse(const uint8_t* z, size_t n, uint64_t* out, size_t cap, uint32_t* level, uint32_t* combined, uint32_t* folded)
{
    if (n < 14 || z[0] != 'B' || z[1] != 'Z' || z[2] != 'h' || z[3] < '1' || z[3] > '9') return -1;
    *level = z[3] - '0';
    uint64_t bit = 32;
    int64_t k = 0;
    uint32_t fold = 0;
    std::vector<uint8_t> bwt(kBzMaxBlock);
    std::vector<BzTables> tt(1);
    for (;;) {
        const uint64_t m = bz_bits48(z, n, bit);
        if (m == kBzEosMagic) break;
        if (m != kBzBlockMagic) return -1;
        BzBits b;
        bb_start(b, z, n, bit + 48);
        const uint32_t crc = bb_take(b, 32);
        bb_fill(b);
        bb_take(b, 1);
        const uint32_t op = bb_take(b, 24);
        bb_fill(b);
        const uint32_t rows = bb_take(b, 16);
        uint32_t nused = 0;
        for (uint32_t i = 0; i < 16; ++i)
            if (rows & (0x8000u >> i)) {
                bb_fill(b);
                nused += (uint32_t)__builtin_popcount(bb_take(b, 16));
            }
        bb_fill(b);
        const uint32_t nt = bb_take(b, 3), nsel = bb_take(b, 15);
        const BzBlockRes r = bz_block_symbols(z, n, bit, bwt.data(), kBzMaxBlock, nullptr, tt[0]);
        if (r.status != kBzOk || r.crc != crc || r.orig_ptr != op) return -1;
        uint32_t longest = 0;
        for (uint32_t g = 0; g < nt; ++g)
            for (uint32_t l = 1; l < 21; ++l)
                if (tt[0].count[g][l]) longest = longest > l ? longest : l;
        if ((size_t)k < cap) {
            uint64_t* o = out + (size_t)k * 8;
            o[0] = bit; o[1] = crc; o[2] = op; o[3] = nt; o[4] = nsel; o[5] = longest; o[6] = r.n; o[7] = nused;
        }
        fold = bz_crc_combine(fold, crc);
        bit = r.end_bit;
        ++k;
    }
    BzBits b;
    bb_start(b, z, n, bit + 48);
    *combined = bb_take(b, 32);
    *folded = fold;
    if ((bit + 80 + 7) / 8 != n) return -1; // nothing behind the padding
    return k;
}

} // extern "C"
