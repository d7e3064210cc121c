// bcj_kernels.h -- launchers of the BCJ filters over byte ranges resident in HBM (bcj_kernels.hip).  Internal.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "bcj_core.h"

namespace snaphash {

constexpr uint32_t kBcjLanes = 256; // a workgroup takes kBcjLanes stretches: a tile of 64 KiB

// A range (one Block): d_base[off .. off + len), any byte alignment, any length, filtered in place as its own Block.
// unit0: the prefix sum of ceil(len / kBcjStretch) over the ranges in front; the table has n + 1 entries, the last one's
// unit0 being the total.
struct BcjRange {
    uint64_t off, len;
    uint32_t unit0;
    uint32_t filter; // kBcjX86 / kBcjArm / kBcjThumb
    uint32_t start;  // the filter's start_offset
    uint32_t encode; // 1 encode, 0 decode
};
static_assert(sizeof(BcjRange) == 32, "BcjRange is 32 bytes");

// bcj_points_kernel (every x86 stretch's first restart point into d_points[0 .. units)), then bcj_apply_kernel (a lane a
// stretch: the x86 owners' walks, the ARM and Thumb words of the stretch).  Nothing outside a range is read or written.
// The first launch is skipped when `any_x86` is false.
hipError_t launch_bcj_ranges(uint8_t* d_base, const BcjRange* d_ranges, uint32_t n, uint32_t units, uint32_t* d_points, bool any_x86,
                             hipStream_t s);

} // namespace snaphash
