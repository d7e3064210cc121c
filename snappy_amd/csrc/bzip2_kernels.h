// bzip2_kernels.h -- launchers of the GPU bzip2 decode (the data.tar.bz2 side; bzip2_kernels.hip).  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bzip2_core.h"

namespace snaphash {

// One linked block of a launch: its slot, its symbol count and origPtr in; the status of the inverse BWT and the
// length of its output after RLE1 out of bz_rle1_count; where that output goes in (bz_rle1_write).
struct BzGpuBlock {
    uint64_t out_off;
    uint64_t out_len;
    uint32_t slot;
    uint32_t n;
    uint32_t orig_ptr;
    int32_t status;
};

constexpr uint32_t kBzChunks = 1024;  // RLE1 chunks of a block at most (one lane each)

// Bit offsets of every block magic in d_in[0..n), appended unordered to d_cand; *d_count counts them all, at most cap
// are written.
hipError_t launch_bz_scan(const uint8_t* d_in, uint64_t n, uint64_t* d_cand, uint32_t* d_count, uint32_t cap, hipStream_t s);
// One workgroup per candidate, lane 0 walking the Huffman stream with the tables in LDS: the block at bit d_starts[i]
// into slot i (kBzMaxBlock bytes of BWT output), its result in d_res[i].
hipError_t launch_bz_symbols(const uint8_t* d_in, uint64_t n, const uint64_t* d_starts, uint32_t count, uint8_t* d_slots,
                             BzBlockRes* d_res, hipStream_t s);
// The inverse BWT of each block, 1024 lanes each: the T vector into d_tt (kBzMaxBlock words a slot) by a stable counting
// sort, then the walk from origPtr split at kBzWalkers sampled positions (bzip2_core.h); the output replaces the BWT
// bytes in the slot.  The status is kBzBad only for a walk that breaks, which a T vector built by the sort cannot do.
hipError_t launch_bz_ibwt(uint8_t* d_slots, uint32_t* d_tt, BzGpuBlock* d_blocks, uint32_t count, hipStream_t s);
// RLE1, first pass: every chunk of every block run from each of the five entry states, the chunks linked; out_len of
// each block and each chunk's entry state and output offset (d_chunks, kBzChunks a slot).
hipError_t launch_bz_rle1_count(const uint8_t* d_slots, BzGpuBlock* d_blocks, uint64_t* d_chunks, uint32_t count, hipStream_t s);
// RLE1, second pass: every chunk's output at d_out + out_off + its offset.
hipError_t launch_bz_rle1_write(const uint8_t* d_slots, const BzGpuBlock* d_blocks, const uint64_t* d_chunks, uint32_t count,
                                uint8_t* d_out, hipStream_t s);

} // namespace snaphash
