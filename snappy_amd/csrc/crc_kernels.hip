// crc_kernels.hip -- CRC-32 (gzip's and bzip2's) and CRC-64/XZ of byte ranges resident in HBM, for gfx950.
//
// The decoded stream of a package sits in HBM (c->inf.d_out) before a single CRC of it can be compared; under
// SNAPHASH_FLAG_GPU_ONLY these kernels take the gzip members' CRC-32s and the bzip2 blocks' CRCs there instead of on
// host threads.  crc_core.h says how a range is cut: tiles of 64 KiB and lane slices of 256 bytes, both laid out from the
// range's end, so that every partial remainder is moved to its place by a constant of its index and the fold is an xor.
//
//   crc_ranges_kernel<KIND>  one workgroup (256 lanes) per (range, tile) in a grid-stride loop.  The eight slice-by-8
//                            tables (8 KiB) are built in LDS, an entry a lane; each lane computes its shift constant
//                            once; per tile a lane runs its slice (16-byte loads between the ragged ends), multiplies by
//                            its constant, and the workgroup xors the 256 products (wave shuffles, then LDS).
//   crc_fold_kernel<KIND>    one workgroup per range: tile remainders times x^(8 * 64 KiB * k), xor'ed; the init and
//                            final xor applied for the range's length.  No atomics, no dependence on completion order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crc_core.h"
#include "crc_kernels.h"

namespace snaphash {

namespace {

__device__ inline uint32_t wave_xor(uint32_t v)
{
    for (int m = 32; m >= 1; m >>= 1) v ^= __shfl_xor(v, m, 64);
    return v;
}

// xor of v over the workgroup's 256 lanes, returned on every lane (red: one word a wave)
__device__ inline uint32_t block_xor(uint32_t v, uint32_t* red)
{
    v = wave_xor(v);
    __syncthreads(); // (red may still be read from the round before)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] ^ red[1] ^ red[2] ^ red[3];
}

template <int KIND>
__global__ __launch_bounds__(kCrcLanes) void crc_ranges_kernel(const uint8_t* base, const uint64_t* offs, const uint64_t* lens,
                                                              const uint32_t* tile0, uint32_t n, uint32_t tile_total,
                                                              uint32_t* partial, CrcPowTable pw)
{
    __shared__ uint32_t tab[8][256];
    __shared__ uint32_t red[4];
    const uint32_t t = threadIdx.x;
    tab[0][t] = crc_table0<KIND>(t);
    __syncthreads();
    uint32_t e = tab[0][t];
    for (int k = 1; k < 8; ++k) {
        e = crc_table_next<KIND>(tab[0], e);
        tab[k][t] = e;
    }
    __syncthreads();
    const uint32_t shift = crc_lane_shift<KIND>(pw, t);
    for (uint32_t pair = blockIdx.x; pair < tile_total; pair += gridDim.x) {
        // the range this tile belongs to: the last r with tile0[r] <= pair (uniform over the workgroup)
        uint32_t lo = 0, hi = n;
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (tile0[mid] <= pair) lo = mid;
            else hi = mid;
        }
        const uint32_t r = lo;
        const uint64_t len = lens[r];
        const uint64_t k = (uint64_t)(tile0[r + 1] - 1 - pair); // counted from the range's end
        uint64_t a, b;
        crc_lane_slice(len, k, t, &a, &b);
        uint32_t c = 0;
        if (b > a) c = crc_mul<KIND>(crc_raw_update<KIND>(tab, 0, base + offs[r] + a, b - a), shift);
        c = block_xor(c, red);
        if (t == 0) partial[pair] = c;
    }
}

template <int KIND>
__global__ __launch_bounds__(kCrcLanes) void crc_fold_kernel(const uint64_t* lens, const uint32_t* tile0, uint32_t n,
                                                            const uint32_t* partial, uint32_t* crcs, CrcPowTable pw)
{
    __shared__ uint32_t red[4];
    const uint32_t t = threadIdx.x;
    const uint32_t step = pw.pw[kCrcTileLog + 8]; // x^(8 * kCrcTile * 256): from a lane's tile to its next
    for (uint32_t r = blockIdx.x; r < n; r += gridDim.x) {
        const uint32_t first = tile0[r], nt = tile0[r + 1] - first;
        uint32_t acc = 0;
        uint32_t m = crc_tile_shift<KIND>(pw, t);
        for (uint32_t k = t; k < nt; k += kCrcLanes) {
            acc ^= crc_mul<KIND>(partial[first + nt - 1 - k], m);
            m = crc_mul<KIND>(m, step);
        }
        acc = block_xor(acc, red);
        // x^(8 len): the product of the constants of len's set bits, a bit a lane of the first wave
        const uint64_t len = lens[r];
        if (t < 64) {
            uint32_t f = (len >> t & 1) ? pw.pw[t] : CrcPoly<KIND>::one;
            for (int q = 32; q >= 1; q >>= 1) f = crc_mul<KIND>(f, __shfl_xor(f, q, 64));
            if (t == 0) crcs[r] = acc ^ crc_mul<KIND>(0xffffffffu, f) ^ 0xffffffffu;
        }
    }
}

template <int KIND> const CrcPowTable& pow_table()
{
    static const CrcPowTable t = [] {
        CrcPowTable x;
        crc_pow_table<KIND>(x);
        return x;
    }();
    return t;
}

// ---- CRC-64/XZ: the same two kernels on 64-bit remainders (tables of 16 KiB in LDS) -------------------------------------

__device__ inline uint64_t block_xor64(uint64_t v, uint32_t* red)
{
    const uint32_t lo = block_xor((uint32_t)v, red), hi = block_xor((uint32_t)(v >> 32), red);
    return (uint64_t)hi << 32 | lo;
}

__global__ __launch_bounds__(kCrcLanes) void crc64_ranges_kernel(const uint8_t* base, const uint64_t* offs, const uint64_t* lens,
                                                                const uint32_t* tile0, uint32_t n, uint32_t tile_total,
                                                                uint64_t* partial, Crc64PowTable pw)
{
    __shared__ uint64_t tab[8][256];
    __shared__ uint32_t red[4];
    const uint32_t t = threadIdx.x;
    tab[0][t] = crc64_table0(t);
    __syncthreads();
    uint64_t e = tab[0][t];
    for (int k = 1; k < 8; ++k) {
        e = crc64_table_next(tab[0], e);
        tab[k][t] = e;
    }
    __syncthreads();
    const uint64_t shift = crc64_lane_shift(pw, t);
    for (uint32_t pair = blockIdx.x; pair < tile_total; pair += gridDim.x) {
        uint32_t lo = 0, hi = n;
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (tile0[mid] <= pair) lo = mid;
            else hi = mid;
        }
        const uint32_t r = lo;
        const uint64_t len = lens[r];
        const uint64_t k = (uint64_t)(tile0[r + 1] - 1 - pair); // counted from the range's end
        uint64_t a, b;
        crc_lane_slice(len, k, t, &a, &b);
        uint64_t c = 0;
        if (b > a) c = crc64_mul(crc64_raw_update(tab, 0, base + offs[r] + a, b - a), shift);
        c = block_xor64(c, red);
        if (t == 0) partial[pair] = c;
    }
}

__global__ __launch_bounds__(kCrcLanes) void crc64_fold_kernel(const uint64_t* lens, const uint32_t* tile0, uint32_t n,
                                                              const uint64_t* partial, uint64_t* crcs, Crc64PowTable pw)
{
    __shared__ uint32_t red[4];
    const uint32_t t = threadIdx.x;
    const uint64_t step = pw.pw[kCrcTileLog + 8]; // x^(8 * kCrcTile * 256): from a lane's tile to its next
    for (uint32_t r = blockIdx.x; r < n; r += gridDim.x) {
        const uint32_t first = tile0[r], nt = tile0[r + 1] - first;
        uint64_t acc = 0;
        uint64_t m = crc64_tile_shift(pw, t);
        for (uint32_t k = t; k < nt; k += kCrcLanes) {
            acc ^= crc64_mul(partial[first + nt - 1 - k], m);
            m = crc64_mul(m, step);
        }
        acc = block_xor64(acc, red);
        if (t == 0) crcs[r] = crc64_finish(pw, acc, lens[r]);
    }
}

const Crc64PowTable& pow_table64()
{
    static const Crc64PowTable t = [] {
        Crc64PowTable x;
        crc64_pow_table(x);
        return x;
    }();
    return t;
}

} // namespace

hipError_t launch_crc_ranges(int kind, const uint8_t* d_base, const uint64_t* d_offs, const uint64_t* d_lens, const uint32_t* d_tile0,
                             uint32_t n, uint32_t tile_total, uint32_t* d_partial, hipStream_t s)
{
    if (n == 0 || tile_total == 0) return hipSuccess;
    const uint32_t grid = tile_total < 4096 ? tile_total : 4096; // 256 CUs x 8 workgroups (8 KiB of LDS each), 16 tiles in a row
    if (kind == kCrcGzip)
        hipLaunchKernelGGL(crc_ranges_kernel<kCrcGzip>, dim3(grid), dim3(kCrcLanes), 0, s, d_base, d_offs, d_lens, d_tile0, n, tile_total,
                           d_partial, pow_table<kCrcGzip>());
    else
        hipLaunchKernelGGL(crc_ranges_kernel<kCrcBzip2>, dim3(grid), dim3(kCrcLanes), 0, s, d_base, d_offs, d_lens, d_tile0, n, tile_total,
                           d_partial, pow_table<kCrcBzip2>());
    return hipGetLastError();
}

hipError_t launch_crc_fold(int kind, const uint64_t* d_lens, const uint32_t* d_tile0, uint32_t n, const uint32_t* d_partial,
                           uint32_t* d_crcs, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    const uint32_t grid = n < 2048 ? n : 2048;
    if (kind == kCrcGzip)
        hipLaunchKernelGGL(crc_fold_kernel<kCrcGzip>, dim3(grid), dim3(kCrcLanes), 0, s, d_lens, d_tile0, n, d_partial, d_crcs,
                           pow_table<kCrcGzip>());
    else
        hipLaunchKernelGGL(crc_fold_kernel<kCrcBzip2>, dim3(grid), dim3(kCrcLanes), 0, s, d_lens, d_tile0, n, d_partial, d_crcs,
                           pow_table<kCrcBzip2>());
    return hipGetLastError();
}

hipError_t launch_crc64_ranges(const uint8_t* d_base, const uint64_t* d_offs, const uint64_t* d_lens, const uint32_t* d_tile0, uint32_t n,
                               uint32_t tile_total, uint64_t* d_partial, hipStream_t s)
{
    if (n == 0 || tile_total == 0) return hipSuccess;
    const uint32_t grid = tile_total < 4096 ? tile_total : 4096;
    hipLaunchKernelGGL(crc64_ranges_kernel, dim3(grid), dim3(kCrcLanes), 0, s, d_base, d_offs, d_lens, d_tile0, n, tile_total, d_partial,
                       pow_table64());
    return hipGetLastError();
}

hipError_t launch_crc64_fold(const uint64_t* d_lens, const uint32_t* d_tile0, uint32_t n, const uint64_t* d_partial, uint64_t* d_crcs,
                             hipStream_t s)
{
    if (n == 0) return hipSuccess;
    const uint32_t grid = n < 2048 ? n : 2048;
    hipLaunchKernelGGL(crc64_fold_kernel, dim3(grid), dim3(kCrcLanes), 0, s, d_lens, d_tile0, n, d_partial, d_crcs, pow_table64());
    return hipGetLastError();
}

} // namespace snaphash
