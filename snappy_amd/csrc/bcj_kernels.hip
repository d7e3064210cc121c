// bcj_kernels.hip -- the .xz format's BCJ filters (x86, PowerPC, IA64, ARM, ARM-Thumb, SPARC) over byte ranges resident in
// HBM, for gfx950, and the launcher of one stage of a filter chain (Delta's kernels: delta_kernels.hip).
//
// On the build side the filter stands between the staging copy and lzma_chains_kernel (xzpack.inc); on the install side,
// under SNAPHASH_FLAG_GPU_ONLY, between lzma2_blocks_kernel and the Check kernels (unxz.inc).  A range is a Block: positions
// count from its first byte.  bcj_core.h says how a Block is cut into stretches of 256 bytes and why the cuts are sound.
//
//   bcj_points_kernel   a lane a stretch of an x86 range: the stretch's first restart point (a position whose five bytes
//                       in front hold no 0xE8 / 0xE9), or none.  Reads only.
//   bcj_apply_kernel    a lane a stretch.  x86: a stretch with a point owns the walk from it to the next owner's point
//                       (found by reading the points of the stretches behind; every gap is read by one owner, so the work
//                       is linear); a stretch without one returns.  The other five: the stretch's words (IA64: bundles), each by its own bytes.
//                       In place: no walk writes at or past the next owner's point, and a word's conversion leaves the
//                       bits its neighbours test as they are.
// Two launches, because the second writes what the first reads across stretch borders.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bcj_core.h"
#include "bcj_kernels.h"

namespace snaphash {

namespace {

// the range unit u belongs to: the last r with unit0[r] <= u (ranges of no unit are stepped over: their unit0 is the next one's)
__device__ inline uint32_t bcj_range_of(const BcjRange* ranges, uint32_t n, uint32_t u)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ranges[mid].unit0 <= u) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kBcjLanes) void bcj_points_kernel(const uint8_t* base, const BcjRange* ranges, uint32_t n, uint32_t units,
                                                              uint32_t* points)
{
    const uint32_t stride = gridDim.x * kBcjLanes;
    for (uint32_t u = blockIdx.x * kBcjLanes + threadIdx.x; u < units; u += stride) {
        const BcjRange r = ranges[bcj_range_of(ranges, n, u)];
        if (r.filter != kBcjX86) continue;
        points[u] = bcj_x86_stretch_point(base + r.off, r.len, u - r.unit0, kBcjStretch);
    }
}

__global__ __launch_bounds__(kBcjLanes) void bcj_apply_kernel(uint8_t* base, const BcjRange* ranges, uint32_t n, uint32_t units,
                                                             const uint32_t* points)
{
    const uint32_t stride = gridDim.x * kBcjLanes;
    for (uint32_t u = blockIdx.x * kBcjLanes + threadIdx.x; u < units; u += stride) {
        const uint32_t ri = bcj_range_of(ranges, n, u);
        const BcjRange r = ranges[ri];
        const uint32_t nk = ranges[ri + 1].unit0 - r.unit0; // (the table's entry n holds the total)
        bcj_stretch_apply(r.filter, r.encode != 0, base + r.off, r.len, u - r.unit0, nk, kBcjStretch, points + r.unit0, r.start);
    }
}

} // namespace

hipError_t launch_xz_filter_stage(const XzFilterStage& t, bool encode, hipStream_t s)
{
    if (t.n == 0 || t.units == 0) return hipSuccess;
    if (t.any_bcj) {
        const uint32_t tiles = (t.units + kBcjLanes - 1) / kBcjLanes;
        const uint32_t grid = tiles < 4096 ? tiles : 4096; // 256 CUs x 16 workgroups; the rest by the grid-stride loops
        if (t.any_x86) {
            hipLaunchKernelGGL(bcj_points_kernel, dim3(grid), dim3(kBcjLanes), 0, s, t.d_base, t.d_ranges, t.n, t.units, t.d_points);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(bcj_apply_kernel, dim3(grid), dim3(kBcjLanes), 0, s, t.d_base, t.d_ranges, t.n, t.units, t.d_points);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return launch_delta_ranges(t, encode, s); // (a range is one or the other: the two sets of kernels touch different ranges)
}

hipError_t launch_bcj_ranges(uint8_t* d_base, const BcjRange* d_ranges, uint32_t n, uint32_t units, uint32_t* d_points, bool any_x86,
                             hipStream_t s)
{
    XzFilterStage t{};
    t.d_base = d_base;
    t.d_ranges = d_ranges;
    t.n = n;
    t.units = units;
    t.d_points = d_points;
    t.any_x86 = any_x86;
    t.any_bcj = true;
    return launch_xz_filter_stage(t, false, s); // (no Delta range: the direction is each range's own)
}

} // namespace snaphash
