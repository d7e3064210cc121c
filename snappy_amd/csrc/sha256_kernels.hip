// sha256_kernels.hip -- SHA-256 of byte ranges resident in HBM, for gfx950 (MI355X, CDNA4): the .xz container's Check
// id 10, read by the install side (unxz.inc) and written by the producer (xzpack.inc), both over bytes that are in HBM
// already.
//
// A range's blocks are one chain, so the parallel axis is the list of ranges and the shape is sha512_wide_kernel's: a
// lane carries a range, a wave 64 of them, a workgroup is one wave.  What differs is where the bytes lie: a range begins
// at any byte address (a Block begins where the Blocks in front of it end), so the wave loads aligned 16-byte words --
// four lanes a range, sixteen ranges a load instruction, four instructions a step -- into a wave-private LDS tile, and a
// lane turns the twenty dwords its block touches (the last aligned word of the block before, kept in registers, and the
// step's four) into sixteen message words by a funnel shift (sha256_core.h sha256_lane_words).  The next step's words
// are loaded into registers while this one is hashed.  Only aligned words that overlap a range are read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sha256_core.h"
#include "sha256_kernels.h"

namespace snaphash {

namespace {

// uint4 a range's row: the carry word's place (written for a tail alone) and the step's four.  Five is odd: the 64 rows'
// ds_read_b128 fall on all banks without a pad word of their own.
constexpr int kRow = 5;
static_assert(kRow * 16 == kSha256TileRow && kSha256Step == kSha256Block && kSha256Load == 16, "the units the tests name");

// the round constants in the constant address space: uniform indexing turns into scalar loads
__constant__ uint32_t d_K256[64] = {SNAPHASH_K256_LIST};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) u32x4* gptr_u4;
__device__ __forceinline__ uint4 load_u4(uint64_t addr) // global_load_dwordx4
{
    const u32x4 v = *(gptr_u4)(uintptr_t)addr;
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ uint32_t shfl_u32(uint32_t v, int src) { return (uint32_t)__shfl((int)v, src, 64); }
__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src)
{
    return ((uint64_t)shfl_u32((uint32_t)(v >> 32), src) << 32) | shfl_u32((uint32_t)v, src);
}

} // namespace

__global__ __launch_bounds__(64) void sha256_ranges_kernel(const uint8_t* __restrict__ base, const Sha256Range* __restrict__ ranges, uint32_t n,
                                                           uint8_t* __restrict__ digests)
{
    __shared__ uint4 tile[64 * kRow];
    const uint32_t lane = threadIdx.x;
    const uint32_t slot = blockIdx.x * 64u + lane;
    const bool have = slot < n;

    uint64_t off = 0, len = 0;
    uint32_t idx = 0;
    if (have) {
        off = ranges[slot].off;
        len = ranges[slot].len;
        idx = ranges[slot].idx;
    }
    const uint64_t addr = (uint64_t)(uintptr_t)base + off;
    const uint32_t sh = (uint32_t)addr & 15u;
    const uint64_t word0 = addr - sh;
    const uint32_t nfull = (uint32_t)(len >> 6), rem = (uint32_t)len & 63u;
    const uint32_t nblk = have ? (uint32_t)sha256_blocks(len) : 0u;
    const uint32_t nw = have ? (uint32_t)sha256_range_words(sh, len) : 0u;

    // the cooperative loader: instruction i covers the ranges 16i .. 16i + 15, lane l fetches the aligned word
    // 4b + 1 + (l & 3) of range 16i + (l >> 2)
    const uint32_t piece = lane & 3u;
    uint64_t tptr[4];
    uint32_t tnw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = 16 * i + (int)(lane >> 2);
        tptr[i] = shfl_u64(word0, t) + 16u * (1u + piece);
        tnw[i] = shfl_u32(nw, t);
    }

    uint32_t H[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) H[k] = IV256[k];

    uint4 carry = make_uint4(0, 0, 0, 0); // the aligned word 4b: the last one of the step before
    if (nw) carry = load_u4(word0);
    uint4 pre[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        pre[i] = make_uint4(0, 0, 0, 0);
        if (1u + piece < tnw[i]) pre[i] = load_u4(tptr[i]);
    }

    for (uint32_t b = 0; __any(b < nblk); ++b) {
        __syncthreads(); // single wave: orders the last step's tile reads before these writes
#pragma unroll
        for (int i = 0; i < 4; ++i) tile[(16 * i + (lane >> 2)) * kRow + 1 + piece] = pre[i];
        __syncthreads();

        // the next step's words while this one is hashed (b + 1 <= 2^29: the word's number fits)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t j = 4u * (b + 1u) + 1u + piece;
            pre[i] = make_uint4(0, 0, 0, 0);
            if (j < tnw[i]) pre[i] = load_u4(tptr[i] + (uint64_t)(b + 1u) * kSha256Step);
        }

        const uint4 q1 = tile[lane * kRow + 1], q2 = tile[lane * kRow + 2], q3 = tile[lane * kRow + 3], q4 = tile[lane * kRow + 4];
        const uint32_t d[20] = {carry.x, carry.y, carry.z, carry.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y,
                                q2.z,    q2.w,    q3.x,    q3.y,    q3.z, q3.w, q4.x, q4.y, q4.z, q4.w};
        uint32_t w[16];
        sha256_lane_words(w, d, sh);
        if (__any(b >= nfull && b < nblk)) { // wave-uniform: only near a range's end
            if (b >= nfull && b < nblk) {
                tile[lane * kRow] = carry; // the block's twenty dwords in one place: the tail reads bytes
                const uint8_t* row = reinterpret_cast<const uint8_t*>(tile + lane * kRow) + sh;
                sha256_tail_block(w, b - nfull, rem, len, [&](uint32_t j) { return (uint32_t)row[j]; });
            }
        }
        sha256_compress(H, w, b < nblk, d_K256);
        carry = q4;
    }

    if (have) {
        uint4* o = reinterpret_cast<uint4*>(digests + (uint64_t)idx * kSha256Digest);
        o[0] = make_uint4(__builtin_bswap32(H[0]), __builtin_bswap32(H[1]), __builtin_bswap32(H[2]), __builtin_bswap32(H[3]));
        o[1] = make_uint4(__builtin_bswap32(H[4]), __builtin_bswap32(H[5]), __builtin_bswap32(H[6]), __builtin_bswap32(H[7]));
    }
}

hipError_t launch_sha256_ranges(const uint8_t* d_base, const Sha256Range* d_ranges, uint32_t n, uint8_t* d_digests, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(sha256_ranges_kernel, dim3((n + 63u) / 64u), dim3(64), 0, s, d_base, d_ranges, n, d_digests);
    return hipGetLastError();
}

} // namespace snaphash
