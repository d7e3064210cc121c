// lzma2_check_kernels.h -- internal interface of the .xz producer's self-check kernel (lzma2_check_kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "lzma2_check_core.h"

namespace snaphash {

// Chunks [c0, c0 + count) of the nch that the staged stream d_in[0 .. n_in) has (nch = ceil(n_in / kLzCheckChunk); Blocks of
// bsize bytes, a multiple of kLzCheckChunk), each against its stretch [d_z_beg[c], d_z_end[c]) of d_z[0 .. n_z).  A workgroup
// a chunk, all at once: count is at most kLzCheckLaunchChunks.  Writes d_verdicts[c] for those chunks and nothing else.
constexpr uint32_t kLzCheckLaunchChunks = 2048; // the producer's launch (kXzEncLaunchChunks): 256 CUs x 8 of the 10 that fit
hipError_t launch_lzma2_check(const uint8_t* d_in, uint64_t n_in, uint64_t bsize, const uint8_t* d_z, uint64_t n_z, const uint64_t* d_z_beg,
                              const uint64_t* d_z_end, uint32_t c0, uint32_t count, uint32_t nch, Lzma2Verdict* d_verdicts, hipStream_t s);

} // namespace snaphash
