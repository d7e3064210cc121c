// bz2_check_kernels.h -- launchers of the .bz2 producer's self-check (bz2_check_kernels.hip).  Internal.
// The check of `count` blocks is four steps on one stream, over the install side's scratch of `count` slots (Bzip2Bufs):
// launch_bz2_check_symbols, launch_bz2_check_link, bzip2_kernels.h's launch_bz_ibwt and launch_bz_rle1_count as they are,
// launch_bz2_check_compare.  d_jobs / d_verdicts: the `count` blocks' table entries and verdicts; slot i is block i's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bz2_check_core.h"
#include "bzip2_kernels.h"

namespace snaphash {

// One workgroup a block, lane 0 walking with the tables in LDS: the block at bit z_beg into slot i (kBzMaxBlock bytes), at
// most 100 000 x level symbols; a block whose table entry is refused is not read and gets a default BzBlockRes.
hipError_t launch_bz2_check_symbols(const uint8_t* d_z, uint64_t n_z, uint64_t n_in, const Bz2CheckJob* d_jobs, uint32_t level, uint32_t count,
                                    uint8_t* d_slots, BzBlockRes* d_res, hipStream_t s);
// One lane a block: bz2_check_link.  Every verdict is written: an early one, or kBz2CheckPending.
hipError_t launch_bz2_check_link(const BzBlockRes* d_res, const Bz2CheckJob* d_jobs, uint64_t n_z, uint64_t n_in, uint32_t level, uint32_t count,
                                 BzGpuBlock* d_blocks, Bz2Verdict* d_verdicts, hipStream_t s);
// 1 024 lanes a block: the pending blocks' RLE1 chunks against d_in[in_off .. in_off + in_len); the final verdicts.
hipError_t launch_bz2_check_compare(const uint8_t* d_slots, const BzGpuBlock* d_blocks, const uint64_t* d_chunks, const uint8_t* d_in,
                                    const Bz2CheckJob* d_jobs, uint32_t count, Bz2Verdict* d_verdicts, hipStream_t s);

} // namespace snaphash
