// deflate_check_kernels.h -- internal interface of the build side's self-check kernel (deflate_check_kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "deflate_check_core.h"

namespace snaphash {

// Chunks [chunk0, chunk0 + count) of the nchunks that the staged stream d_in[0..n_in) has, each against its stretch of
// d_z[0..z_total): [d_z_off[c], d_z_off[c + 1]) when d_z_sizes is null (the table then has nchunks + 1 entries), else
// [d_z_off[c], d_z_off[c] + d_z_sizes[c]).  last_is_final: chunk nchunks - 1 ends with the member's final block.
// Writes d_verdicts[c] for those chunks and nothing else.
hipError_t launch_deflate_check(const uint8_t* d_in, uint64_t n_in, const uint8_t* d_z, uint64_t z_total, const uint64_t* d_z_off,
                                const uint32_t* d_z_sizes, uint32_t chunk0, uint32_t count, uint32_t nchunks, bool last_is_final,
                                DfCheckVerdict* d_verdicts, hipStream_t s);

} // namespace snaphash
