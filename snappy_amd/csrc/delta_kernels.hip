// delta_kernels.hip -- the .xz format's Delta filter over byte ranges resident in HBM, for gfx950, over the range tables of
// bcj_kernels.h: a Delta range's `start` is its distance d.  delta_core.h says how a Block is cut into tiles of 64 KiB, how a
// tile's 256 lanes share its columns and rows, and why no pass reads what another workgroup of the same pass writes.
//
// A workgroup takes one tile; the grid is the number of tiles of the table (d_tile0), and a tile of a range that is not
// Delta's at this stage returns.  No workgroup waits for another: the scan across tiles is separate launches.
//
//   decode   delta_sums_kernel    a tile's column sums into scratch, d bytes a tile (at kDeltaTail bytes a tile).  Reads only.
//            delta_carry_kernel   a workgroup a range, lane c < d: the range's tiles in order, each tile's sums turned into the
//                                 sum of the tiles in front of it.
//            delta_apply_kernel   a tile's running sums seeded with its carry, in place.
//   encode   delta_tails_kernel   every whole tile's last kDeltaTail bytes into scratch.  Reads only.
//            delta_encode_kernel  a tile from its end to its start in slabs of 4 KiB: the slab's bytes and their bytes in front
//                                 (the tile's own, or the saved tail of the tile in front) are read, then the slab is written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bcj_kernels.h"

namespace snaphash {

namespace {

// the range tile w belongs to: the last r with tile0[r] <= w (ranges of no tile are stepped over: their tile0 is the next one's)
__device__ inline uint32_t delta_range_of(const uint32_t* tile0, uint32_t n, uint32_t w)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (tile0[mid] <= w) lo = mid;
        else hi = mid;
    }
    return lo;
}

// A workgroup's tile: the Block b[0 .. len), the tile [s, e) of it, the distance, and the tile's number in its range.
struct DeltaTileOf {
    uint8_t* b;
    uint64_t s, e;
    uint32_t d, t;
    bool mine; // a Delta range's
};
__device__ inline DeltaTileOf delta_tile_of(uint8_t* base, const BcjRange* ranges, const uint32_t* tile0, uint32_t n, uint32_t w)
{
    const uint32_t ri = delta_range_of(tile0, n, w);
    const BcjRange r = ranges[ri];
    DeltaTileOf T;
    T.mine = r.filter == kXzDelta;
    T.b = base + r.off;
    T.d = r.start;
    T.t = w - tile0[ri];
    T.s = (uint64_t)T.t * kDeltaTile;
    T.e = T.s + kDeltaTile < r.len ? T.s + kDeltaTile : r.len;
    return T;
}

__global__ __launch_bounds__(kDeltaLanes) void delta_sums_kernel(uint8_t* base, const BcjRange* ranges, const uint32_t* tile0, uint32_t n,
                                                                uint8_t* scratch)
{
    __shared__ uint8_t part[kDeltaLanes];
    const DeltaTileOf T = delta_tile_of(base, ranges, tile0, n, blockIdx.x);
    if (!T.mine) return; // (the whole workgroup)
    const uint32_t lane = threadIdx.x;
    part[lane] = delta_lane_sum(T.b, T.s, T.e, T.d, delta_lane(T.s, T.e, T.d, kDeltaLanes, lane));
    __syncthreads();
    if (lane < T.d) scratch[(uint64_t)blockIdx.x * kDeltaTail + lane] = delta_tile_total(part, T.d, kDeltaLanes, lane);
}

__global__ __launch_bounds__(kDeltaLanes) void delta_carry_kernel(const BcjRange* ranges, const uint32_t* tile0, uint8_t* scratch)
{
    const BcjRange r = ranges[blockIdx.x];
    if (r.filter != kXzDelta || threadIdx.x >= r.start) return;
    const uint32_t t0 = tile0[blockIdx.x];
    delta_carry_column(scratch + (uint64_t)t0 * kDeltaTail, tile0[blockIdx.x + 1] - t0, kDeltaTail, threadIdx.x);
}

__global__ __launch_bounds__(kDeltaLanes) void delta_apply_kernel(uint8_t* base, const BcjRange* ranges, const uint32_t* tile0, uint32_t n,
                                                                 const uint8_t* scratch)
{
    __shared__ uint8_t part[kDeltaLanes];
    const DeltaTileOf T = delta_tile_of(base, ranges, tile0, n, blockIdx.x);
    if (!T.mine) return;
    const uint32_t lane = threadIdx.x;
    const DeltaLane L = delta_lane(T.s, T.e, T.d, kDeltaLanes, lane);
    part[lane] = delta_lane_sum(T.b, T.s, T.e, T.d, L);
    __syncthreads();
    if (L.ra == L.rb) return; // (no barrier behind this)
    delta_lane_apply(T.b, T.s, T.e, T.d, L, delta_lane_seed(part, T.d, lane, scratch[(uint64_t)blockIdx.x * kDeltaTail + L.c]));
}

__global__ __launch_bounds__(kDeltaLanes) void delta_tails_kernel(uint8_t* base, const BcjRange* ranges, const uint32_t* tile0, uint32_t n,
                                                                 uint8_t* scratch)
{
    const DeltaTileOf T = delta_tile_of(base, ranges, tile0, n, blockIdx.x);
    if (!T.mine || T.e - T.s < kDeltaTile) return; // (a range's last, partial tile has none behind it)
    scratch[(uint64_t)blockIdx.x * kDeltaTail + threadIdx.x] = delta_tail_byte(T.b, T.e, threadIdx.x);
}

__global__ __launch_bounds__(kDeltaLanes) void delta_encode_kernel(uint8_t* base, const BcjRange* ranges, const uint32_t* tile0, uint32_t n,
                                                                  const uint8_t* scratch)
{
    const DeltaTileOf T = delta_tile_of(base, ranges, tile0, n, blockIdx.x);
    if (!T.mine) return;
    // (tile 0 of a range never reads a tail: its bytes in front are the Block's, 0)
    const uint8_t* tail = scratch + (uint64_t)(blockIdx.x - (T.t ? 1u : 0u)) * kDeltaTail;
    constexpr uint32_t slab = kDeltaLanes * kDeltaSlab;
    const uint32_t nslab = (uint32_t)((T.e - T.s + slab - 1) / slab);
    for (uint32_t k = nslab; k-- > 0;) { // (the same count for every lane: the barrier is reached by all)
        const uint64_t i0 = T.s + (uint64_t)k * slab + threadIdx.x;
        uint8_t out[kDeltaSlab];
#pragma unroll
        for (uint32_t u = 0; u < kDeltaSlab; ++u) {
            const uint64_t i = i0 + u * kDeltaLanes;
            out[u] = i < T.e ? (uint8_t)(T.b[i] - delta_byte_in_front(T.b, i, T.d, T.s, tail)) : 0;
        }
        __syncthreads(); // every read of this slab and of the kDeltaTail bytes in front of it is done
#pragma unroll
        for (uint32_t u = 0; u < kDeltaSlab; ++u) {
            const uint64_t i = i0 + u * kDeltaLanes;
            if (i < T.e) T.b[i] = out[u];
        }
    }
}

} // namespace

hipError_t launch_delta_ranges(const XzFilterStage& t, bool encode, hipStream_t s)
{
    if (!t.any_delta || t.n == 0 || t.tiles == 0) return hipSuccess;
    const dim3 grid(t.tiles), lanes(kDeltaLanes); // a workgroup a tile: no second round
    if (encode) {
        hipLaunchKernelGGL(delta_tails_kernel, grid, lanes, 0, s, t.d_base, t.d_ranges, t.d_tile0, t.n, t.d_delta);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(delta_encode_kernel, grid, lanes, 0, s, t.d_base, t.d_ranges, t.d_tile0, t.n, t.d_delta);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(delta_sums_kernel, grid, lanes, 0, s, t.d_base, t.d_ranges, t.d_tile0, t.n, t.d_delta);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(delta_carry_kernel, dim3(t.n), lanes, 0, s, t.d_ranges, t.d_tile0, t.d_delta);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(delta_apply_kernel, grid, lanes, 0, s, t.d_base, t.d_ranges, t.d_tile0, t.n, t.d_delta);
    return hipGetLastError();
}

} // namespace snaphash
