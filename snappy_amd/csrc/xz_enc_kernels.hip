// xz_enc_kernels.hip -- the LZMA2 encoder on gfx950: the routines of xz_enc_core.h, spread over the chip where the format
// lets them be.  A .xz Block needs nothing of another Block, and a chunk that resets the coder state needs nothing of
// another chunk but the Block's bytes in front of it, which are all known before the first symbol is coded.
//
//   lzma_chains_kernel   a 64-lane workgroup a Block.  The hash chains of the whole Block into HBM, tile (64 positions) by
//                        tile in input order: every lane takes head[h] for its position, signs head[h] with its own
//                        position, and the lanes of a tile that share a hash are linked among themselves by one ballot a
//                        hash.  Budget: the head table, 2^15 words = 128 KiB of LDS, one workgroup a CU; a dozen VGPRs.
//   lzma2_chunks_kernel  a 256-lane workgroup a chunk of 65 536 bytes, every chunk of the launch resident at once (no
//                        grid-stride loop: the launcher refuses more than kXzEncLaunchChunks).  All lanes walk the
//                        chains and leave the best (length, distance) per position in HBM; then lane 0 runs the parse,
//                        the symbol coder and the adaptive range encoder (xzenc_chunk, the very function the host model
//                        runs) with the probabilities in LDS, reset by all lanes.  Budget: 7 990 probabilities = 15 980
//                        bytes of LDS and nothing else there, eight workgroups a CU and more; the serial loop keeps its
//                        coder registers (low, range, cache, four reps, state) in VGPRs: 32 of them, no scratch.
//   lzma2_chunks_priced_kernel   level 1, the same grid: all lanes leave kXzEncCands candidates per
//                        position in HBM (kXzEncDepthHigh links), then all lanes run xzenc_chunk_priced: a window's nodes are
//                        relaxed a lane a target length, lane 0 prices the literal, walks the chosen edges back and codes them.
//                        Budget: the probabilities (15 980 bytes), the window's 1 025 nodes of 28 bytes (28 700), their
//                        forward links (2 050) and the price tables (4 992) = 51 730 bytes of LDS with the two flag words:
//                        three workgroups a CU of 160 KiB.  The chunks of a launch need not all be resident: no workgroup
//                        waits for another.  One barrier a position, three a window.
//   lzma2_concat_kernel  a workgroup a chunk: header and body to their place in the Block's data.
//
// Bytes that one lane stores and another reads -- the candidates the waves leave for lane 0, the heads one tile leaves
// for the next -- have __syncthreads() between the store and the load: a workgroup-scope fence on both sides, as
// xz_kernels.hip explains for the decoder.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "xz_enc_core.h"
#include "xz_enc_kernels.h"

namespace snaphash {

namespace {

constexpr uint32_t kChunkLanes = 256;

__global__ __launch_bounds__(64) void lzma_chains_kernel(const uint8_t* in, uint64_t n, uint32_t bsize, uint32_t* prev)
{
    __shared__ uint32_t head[1u << kXzEncHashBits];
    const uint32_t lane = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * bsize;
    if (base >= n) return;
    const uint32_t blen = (uint32_t)(n - base < bsize ? n - base : bsize);
    const uint8_t* blk = in + base;
    uint32_t* pv = prev + base;
    for (uint32_t i = lane; i < (1u << kXzEncHashBits); i += 64) head[i] = kXzEncNone;
    __syncthreads();
    for (uint32_t t0 = 0; t0 < blen; t0 += 64) { // (uniform: every lane runs every tile)
        const uint32_t p = t0 + lane;
        const bool valid = p + 4 <= blen && p + 4 > p;
        const uint32_t h = valid ? xzenc_hash(xzenc_ld32(blk + p)) : 0;
        uint32_t link = valid ? head[h] : kXzEncNone; // what the tiles in front left
        __syncthreads();
        if (valid) head[h] = p; // one lane of every hash wins
        __syncthreads();
        const bool lost = valid && head[h] != p; // this lane has company in its tile
        uint64_t todo = __ballot(lost);
        while (todo) { // (uniform)
            const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
            const uint32_t hl = (uint32_t)__shfl((int)h, (int)leader, 64);
            const uint64_t m = __ballot(valid && h == hl);
            if (valid && h == hl) {
                const uint64_t lower = m & ((1ull << lane) - 1ull);
                if (lower) link = t0 + 63u - (uint32_t)__builtin_clzll(lower);
                if (((m >> lane) >> 1) == 0ull) head[h] = p; // the tile's last position of this hash
            }
            todo &= ~m;
        }
        if (p < blen) pv[p] = link;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kChunkLanes) void lzma2_chunks_kernel(const uint8_t* in, uint64_t n, uint32_t bsize, const uint32_t* prev,
                                                                    uint32_t* cand, uint8_t* slots, uint32_t* res, uint32_t c0, uint32_t count)
{
    __shared__ uint16_t probs[kXzEncProbs];
    if (blockIdx.x >= count) return;
    const uint32_t ci = c0 + blockIdx.x;
    const uint64_t at = (uint64_t)ci * kXzEncChunk;
    if (at >= n) return;
    const uint64_t base = at - at % bsize; // the chunk's Block
    const uint32_t blen = (uint32_t)(n - base < bsize ? n - base : bsize);
    const uint32_t cs = (uint32_t)(at - base);
    const uint32_t ce = cs + kXzEncChunk < blen ? cs + kXzEncChunk : blen;
    const uint8_t* blk = in + base;
    const uint32_t* pv = prev + base;
    uint32_t* cd = cand + base;
    for (uint32_t i = threadIdx.x; i < kXzEncProbs; i += kChunkLanes) probs[i] = (uint16_t)kLzmaProbInit;
    for (uint32_t p = cs + threadIdx.x; p < ce; p += kChunkLanes) cd[p] = xzenc_find(blk, pv, p, ce);
    __syncthreads();
    if (threadIdx.x == 0) {
        NoEncOps ops;
        res[ci] = xzenc_chunk(blk, cs, ce, cd, probs, slots + (uint64_t)ci * kXzEncSlot, kXzEncSlot, ops);
    }
}

// the kernel's lanes for xzenc_chunk_priced: a thread a lane, the workgroup's barrier between what one stores and another loads
struct XzEncGroupLanes {
    template <class F> __device__ __forceinline__ void each(F&& f) { f(threadIdx.x); }
    __device__ __forceinline__ bool first() const { return threadIdx.x == 0; }
    __device__ __forceinline__ void sync() { __syncthreads(); }
};
static_assert(kChunkLanes == kXzEncLanes, "a thread a lane of the parse");

// Level 1: kXzEncCands candidates a position by all lanes, then xzenc_chunk_priced, the function the host model runs, by
// all lanes: the relaxation of a node's edges a lane a target length, the coder on lane 0.
__global__ __launch_bounds__(kChunkLanes) void lzma2_chunks_priced_kernel(const uint8_t* in, uint64_t n, uint32_t bsize, const uint32_t* prev,
                                                                           uint32_t* cand, uint8_t* slots, uint32_t* res, uint32_t c0, uint32_t count)
{
    __shared__ uint16_t probs[kXzEncProbs];
    __shared__ XzEncWork work;
    if (blockIdx.x >= count) return;
    const uint32_t ci = c0 + blockIdx.x;
    const uint64_t at = (uint64_t)ci * kXzEncChunk;
    if (at >= n) return;
    const uint64_t base = at - at % bsize; // the chunk's Block
    const uint32_t blen = (uint32_t)(n - base < bsize ? n - base : bsize);
    const uint32_t cs = (uint32_t)(at - base);
    const uint32_t ce = cs + kXzEncChunk < blen ? cs + kXzEncChunk : blen;
    const uint8_t* blk = in + base;
    const uint32_t* pv = prev + base;
    uint32_t* cd = cand + base * kXzEncCands;
    for (uint32_t i = threadIdx.x; i < kXzEncProbs; i += kChunkLanes) probs[i] = (uint16_t)kLzmaProbInit;
    for (uint32_t p = cs + threadIdx.x; p < ce; p += kChunkLanes) xzenc_find_set(blk, pv, p, ce, cd + (uint64_t)p * kXzEncCands);
    __syncthreads();
    NoEncOps ops;
    XzEncGroupLanes ln;
    const uint32_t r = xzenc_chunk_priced(blk, cs, ce, cd, probs, work, slots + (uint64_t)ci * kXzEncSlot, kXzEncSlot, ops, ln);
    if (threadIdx.x == 0) res[ci] = r;
}

__global__ __launch_bounds__(kChunkLanes) void lzma2_concat_kernel(const uint8_t* in, uint64_t n, uint32_t bsize, const uint8_t* slots,
                                                                    const uint32_t* res, const uint64_t* dst, uint8_t* out, uint32_t nch)
{
    const uint32_t ci = blockIdx.x;
    if (ci >= nch) return;
    const uint64_t at = (uint64_t)ci * kXzEncChunk;
    if (at >= n) return;
    const uint32_t usize = (uint32_t)(n - at < kXzEncChunk ? n - at : kXzEncChunk);
    const uint32_t r = res[ci];
    const bool first = at % bsize == 0;
    const bool last = (at + kXzEncChunk) % bsize == 0 || at + kXzEncChunk >= n;
    const bool stored = r == kXzEncStored;
    const uint32_t len = stored ? usize : (r <= kXzEncChunk ? r : 0u); // (the host has refused an impossible result already)
    const uint8_t* src = stored ? in + at : slots + (uint64_t)ci * kXzEncSlot;
    uint8_t* d = out + dst[ci];
    uint32_t hdr = stored ? 3u : 6u;
    if (threadIdx.x == 0) {
        uint8_t h[6];
        hdr = xzenc_chunk_header(h, first, usize, r);
        for (uint32_t k = 0; k < hdr; ++k) d[k] = h[k];
        if (last) d[hdr + len] = 0; // the Block's end byte
    }
    for (uint32_t i = threadIdx.x; i < len; i += kChunkLanes) d[hdr + i] = src[i];
}

} // namespace

hipError_t launch_lzma_chains(const uint8_t* d_in, uint64_t n, uint32_t bsize, uint32_t* d_prev, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (bsize == 0 || bsize % kXzEncChunk || bsize > kXzEncBlockMax) return hipErrorInvalidValue;
    const uint64_t nb = (n + bsize - 1) / bsize;
    if (nb > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lzma_chains_kernel, dim3((uint32_t)nb), dim3(64), 0, s, d_in, n, bsize, d_prev);
    return hipGetLastError();
}

hipError_t launch_lzma2_chunks(const uint8_t* d_in, uint64_t n, uint32_t bsize, const uint32_t* d_prev, uint32_t* d_cand, uint8_t* d_slots,
                               uint32_t* d_res, uint32_t c0, uint32_t count, hipStream_t s, uint32_t level)
{
    if (count == 0) return hipSuccess;
    if (bsize == 0 || bsize % kXzEncChunk || bsize > kXzEncBlockMax || count > kXzEncLaunchChunks || level > kXzEncLevelMax) return hipErrorInvalidValue;
    if (((uint64_t)c0 + count - 1) * kXzEncChunk >= n) return hipErrorInvalidValue; // a chunk behind the piece
    if (level) hipLaunchKernelGGL(lzma2_chunks_priced_kernel, dim3(count), dim3(kChunkLanes), 0, s, d_in, n, bsize, d_prev, d_cand, d_slots, d_res, c0, count);
    else hipLaunchKernelGGL(lzma2_chunks_kernel, dim3(count), dim3(kChunkLanes), 0, s, d_in, n, bsize, d_prev, d_cand, d_slots, d_res, c0, count);
    return hipGetLastError();
}

hipError_t launch_lzma2_concat(const uint8_t* d_in, uint64_t n, uint32_t bsize, const uint8_t* d_slots, const uint32_t* d_res,
                               const uint64_t* d_dst, uint8_t* d_out, uint32_t nch, hipStream_t s)
{
    if (nch == 0) return hipSuccess;
    if (bsize == 0 || bsize % kXzEncChunk || ((uint64_t)nch - 1) * kXzEncChunk >= n) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lzma2_concat_kernel, dim3(nch), dim3(kChunkLanes), 0, s, d_in, n, bsize, d_slots, d_res, d_dst, d_out, nch);
    return hipGetLastError();
}

} // namespace snaphash
