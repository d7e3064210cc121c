// bzip2_enc_kernels.h -- launchers of the GPU bzip2 encoder (bzip2_enc_kernels.hip; bzpack.inc drives them).  Internal.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "bzip2_enc_core.h"

namespace snaphash {

constexpr uint32_t kBzEncSelStride = 18048;              // selectors a block, >= kBzMaxSelectors
constexpr uint64_t kBzEncLaunchBytes = 32ull * 899840;   // BWT bytes of one launch's blocks together: 32 blocks at level 9
constexpr uint32_t kBzEncLaunchBlocksMax = 1024;         // and never more blocks than this
constexpr uint32_t kBzEncScratchPerByte = 28;            // keys (2 x 8), indices (2 x 4), ranks (4) of the sort, a BWT byte

// one piece of the staged slot: where it is, its length (1 .. bzenc_piece(level)), its CRC (crc_kernels.hip)
struct BzEncJob {
    uint64_t in_off;
    uint32_t in_len;
    uint32_t crc;
};
// a range the BWT kernel sorts, and where its last column goes
struct BzBwtJob {
    uint64_t in_off, out_off;
    uint32_t n, pad;
};
// what the stages left of one block
struct BzEncRes {
    uint32_t rle_n, orig_ptr, nmtf, bits; // bits: the block's length in its output slot
    uint32_t over, pad;                   // over: a stage met its buffer's end (by construction none does)
};

// The scratch of one launch, every array `blocks` x its stride: cap is the longest BWT input a block may have.
struct BzEncScratch {
    uint32_t cap;          // bytes a block after RLE1, at most (a multiple of 64)
    uint32_t slot_words;   // bzenc_slot_words(cap)
    uint8_t *rle, *last;   // cap + 64 a block
    uint64_t *key_a, *key_b;
    uint32_t *idx_a, *idx_b, *rank; // cap a block
    uint16_t* syms;        // cap + 64 a block
    BzEncMap* maps;
    uint8_t* sel;          // kBzEncSelStride a block
    uint32_t* slots;       // slot_words a block, zeroed by the launcher
    BzBwtJob* bwt_jobs;
    BzEncRes* res;
};

// RLE1, BWT, MTF and coding of nblk pieces of d_in (jobs: nblk entries in HBM).  ev: null, or five events recorded before
// and after each of the four stages.
hipError_t launch_bzenc_blocks(const uint8_t* d_in, const BzEncJob* d_jobs, const BzEncScratch& s, uint32_t nblk, hipStream_t st, hipEvent_t* ev);
// The same launch entered behind its second stage (snaphash_bzenc_stages_device's from_last mode): MTF and coding of nblk
// last columns the caller has put into s.last, with s.res[k].rle_n (1 .. s.cap) and .orig_ptr set and the other fields of
// s.res zero; of d_jobs only the CRCs are read.
hipError_t launch_bzenc_from_last(const BzEncJob* d_jobs, const BzEncScratch& s, uint32_t nblk, hipStream_t st);
// the BWT stage alone over nblk ranges (jobs in HBM, every n <= s.cap): last columns to d_out, origPtr to d_op[0..nblk)
hipError_t launch_bzenc_bwt(const uint8_t* d_in, const BzBwtJob* d_jobs, uint8_t* d_out, uint32_t* d_op, const BzEncScratch& s, uint32_t nblk,
                            hipStream_t st);
// shifts the blocks' bits together: block k's res.bits bits go to bit d_dst[k] of d_out (zeroed by the launcher for
// out_words words); carry: the bits (carry_bits < 8 of them, left-aligned in a byte) that precede block 0 in byte 0
hipError_t launch_bzenc_concat(const BzEncScratch& s, const uint64_t* d_dst, uint32_t nblk, uint32_t* d_out, uint64_t out_words, uint32_t carry,
                               hipStream_t st);

} // namespace snaphash
