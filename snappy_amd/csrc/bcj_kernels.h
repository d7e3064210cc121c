// bcj_kernels.h -- launchers of the .xz filters over byte ranges resident in HBM: the BCJ filters (bcj_kernels.hip) and Delta
// (delta_kernels.hip).  Internal.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "bcj_core.h"
#include "delta_core.h"

namespace snaphash {

constexpr uint32_t kBcjLanes = 256; // a workgroup takes kBcjLanes stretches: a tile of 64 KiB

// A range (one Block): d_base[off .. off + len), any byte alignment, any length, filtered in place as its own Block.
// unit0: the prefix sum of ceil(len / kBcjStretch) over the ranges in front; the table has n + 1 entries, the last one's
// unit0 being the total.
struct BcjRange {
    uint64_t off, len;
    uint32_t unit0;
    uint32_t filter; // one of the six BCJ ids, kXzDelta, or 0: the range has no filter at this stage and is skipped
    uint32_t start;  // the filter's start_offset; for kXzDelta the distance, 1 .. 256
    uint32_t encode; // 1 encode, 0 decode
};
static_assert(sizeof(BcjRange) == 32, "BcjRange is 32 bytes");

// bcj_points_kernel (every x86 stretch's first restart point into d_points[0 .. units)), then bcj_apply_kernel (a lane a
// stretch: the x86 owners' walks, the words and bundles of the other five).  Nothing outside a range is read or written.
// The first launch is skipped when `any_x86` is false.
hipError_t launch_bcj_ranges(uint8_t* d_base, const BcjRange* d_ranges, uint32_t n, uint32_t units, uint32_t* d_points, bool any_x86,
                             hipStream_t s);

// One stage of a filter chain over a table: every range's filter at this stage, in place.  A chain of k filters is k stages
// (encode: the header's first filter first; decode: the one nearest LZMA2 first), each with the table's filter and start
// set for it.
struct XzFilterStage {
    uint8_t* d_base;
    const BcjRange* d_ranges; // n + 1 entries
    uint32_t n, units;
    uint32_t* d_points;       // units words: x86's restart points
    bool any_x86, any_bcj, any_delta; // an x86 range; a range of any BCJ filter; a Delta range
    // Delta ranges alone need what follows
    const uint32_t* d_tile0;  // n + 1 entries: the prefix sum of ceil(len / kDeltaTile) over ALL ranges, the last the total
    uint32_t tiles;
    uint8_t* d_delta;         // tiles * kDeltaTail bytes: the tiles' column sums and carries (decode), their tails (encode)
};
// The BCJ ranges by launch_bcj_ranges' two kernels; the Delta ranges by delta_sums_kernel, delta_carry_kernel and
// delta_apply_kernel (decode) or delta_tails_kernel and delta_encode_kernel (encode): a workgroup a tile, no workgroup
// waiting for another.  Every Delta range of the stage runs in `encode`'s direction.
hipError_t launch_xz_filter_stage(const XzFilterStage& t, bool encode, hipStream_t s);
// how many kernels that launches
inline uint32_t xz_filter_stage_launches(const XzFilterStage& t, bool encode)
{
    return (t.any_bcj ? (t.any_x86 ? 2u : 1u) : 0u) + (t.any_delta && t.tiles ? (encode ? 2u : 3u) : 0u);
}

// delta_kernels.hip: the Delta ranges of a stage (launch_xz_filter_stage calls it)
hipError_t launch_delta_ranges(const XzFilterStage& t, bool encode, hipStream_t s);

} // namespace snaphash
