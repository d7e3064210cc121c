// xz_enc_kernels.h -- launchers of the LZMA2 encoder's kernels (xz_enc_kernels.hip).  Internal.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "xz_enc_core.h"

namespace snaphash {

// The staged piece d_in[0 .. n) is cut into Blocks of bsize bytes (a multiple of kXzEncChunk; the last Block may be short)
// and chunks of kXzEncChunk bytes; chunk i covers d_in[i * kXzEncChunk ..) and belongs to Block i / (bsize / kXzEncChunk).

// d_prev[p] (a word per byte of the piece): the nearest earlier position of p's Block with the same hash, relative to the
// Block, or kXzEncNone.  A 64-lane workgroup a Block.
hipError_t launch_lzma_chains(const uint8_t* d_in, uint64_t n, uint32_t bsize, uint32_t* d_prev, hipStream_t s);

// Chunks c0 .. c0 + count of the piece, a workgroup each, all at once: count is at most kXzEncLaunchChunks.  d_cand: a
// word per byte of the piece (the candidates); d_slots: kXzEncSlot bytes a chunk (the coder's output); d_res[i]: the
// chunk's csize, or kXzEncStored.  Nothing else is written.  level 1 (lzma2_chunks_priced_kernel): d_cand holds
// kXzEncCands words per byte of the piece.
constexpr uint32_t kXzEncLaunchChunks = 2048; // 256 CUs x 8 workgroups of 16 KB of LDS: what is resident at once
// what the producer puts into one launch at level 1: 256 CUs x 3 workgroups of 51 KB of LDS are resident at once, and a launch
// of no more lasts as long as its slowest chunk (DESIGN.md sec. 27 holds that against sec. 17's one-second bound)
constexpr uint32_t kXzEncLaunchChunksPriced = 768;
hipError_t launch_lzma2_chunks(const uint8_t* d_in, uint64_t n, uint32_t bsize, const uint32_t* d_prev, uint32_t* d_cand, uint8_t* d_slots,
                               uint32_t* d_res, uint32_t c0, uint32_t count, hipStream_t s, uint32_t level = 0);

// Chunk i's header and body (from its slot, or -- stored -- from the input) to d_out + d_dst[i], and the Block's end byte
// behind a Block's last chunk.  nch: all chunks of the piece.
hipError_t launch_lzma2_concat(const uint8_t* d_in, uint64_t n, uint32_t bsize, const uint8_t* d_slots, const uint32_t* d_res,
                               const uint64_t* d_dst, uint8_t* d_out, uint32_t nch, hipStream_t s);

} // namespace snaphash
