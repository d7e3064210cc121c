// lzma2_check_kernels.hip -- the .xz producer's self-check on gfx950: while a slot is being compressed the
// staged tar stream and the assembled LZMA2 chunks are both in HBM, so whether the one decodes back to the other is decided
// there, before a byte travels to the host.  lzma2_check_core.h holds the walk; here a 64-lane workgroup takes one 64 KiB
// chunk.  The walk through a range-coded stream is one serial chain, so lane 0 runs xz_core.h's decoder with the
// probabilities in LDS -- 7 990 of them, the producer's lc=3 lp=0 alone: 15 980 bytes, ten workgroups a CU by LDS (eight by
// the registers the compiler takes), so the 2 048 chunks of a producer launch are resident at once on 256 CUs (sized for
// kLzmaProbsMax it would be five, and they would not be) -- and the compressed bytes prefetched sixteen at a time.  What
// the wave adds is width where there is some: the probabilities are reset by all lanes, and match bodies (up to 273 byte
// pairs) and stored chunks are compared by all lanes, a round of 64 at a time; the verdict names the FIRST differing byte,
// the lowest lane of the first round whose ballot is not empty, which is the byte the host walker names.  Nothing is
// written but the chunk's verdict, so the decoder's barriers between lane 0's stores and the wave's copies have no
// counterpart here: the one barrier is behind the probabilities' reset.
// Integer work with data-dependent control flow: no MFMA.  Not HBM-bound: a chunk is one lane's serial chain.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lzma2_check_core.h"
#include "lzma2_check_kernels.h"

namespace snaphash {

namespace {

// Lzma2CheckIO with XzDevIO's fetch: sixteen compressed bytes at a time where they are aligned and lie inside the stretch
struct Lzma2CheckDevIO {
    const uint8_t* z;
    const uint8_t* in;
    uint64_t ip, iend;
    uint64_t diff_at;
    bool ov, diff;
    uint64_t lim; // the stretch's end: no load goes past it
    uint4 buf;    // z[buf_at .. buf_at + 16)
    uint64_t buf_at;
    __device__ uint32_t in_at(uint64_t p) const { return z[p]; }
    __device__ uint32_t next()
    {
        if (ip >= iend) {
            ov = true;
            return 0;
        }
        const uint64_t i = ip++;
        uint64_t k = i - buf_at;
        if (k >= 16) {
            if ((((uintptr_t)(z + i)) & 15) != 0 || lim - i < 16) return z[i];
            buf = *(const uint4*)(z + i);
            buf_at = i;
            k = 0;
        }
        const uint32_t w = k < 8 ? (k < 4 ? buf.x : buf.y) : (k < 12 ? buf.z : buf.w);
        return (w >> (8 * ((uint32_t)k & 3))) & 0xff;
    }
    __device__ bool over() const { return ov || diff; }
    __device__ uint32_t out_at(uint64_t p) const { return in[p]; }
    __device__ void put(uint64_t p, uint32_t b)
    {
        if (!ov && !diff && in[p] != (uint8_t)b) {
            diff = true;
            diff_at = p;
        }
    }
};

__device__ inline uint64_t shfl0_u64(uint64_t v)
{
    const uint32_t lo = __shfl((uint32_t)v, 0, 64), hi = __shfl((uint32_t)(v >> 32), 0, 64);
    return (uint64_t)hi << 32 | lo;
}

// The walk's steps for a wave: every lane is in every step (the walk's branches are taken on values that are the same on
// all lanes: the header's bytes, and what the steps below hand back), lane 0 alone holds the coder's true state.
struct Lzma2CheckWaveWalk {
    uint32_t lane;
    __device__ void reset(uint16_t* probs)
    {
        for (uint32_t i = lane; i < kLzCheckProbs; i += 64) probs[i] = (uint16_t)kLzmaProbInit;
        __syncthreads();
    }
    __device__ bool start(LzmaDec& d, Lzma2CheckDevIO& io)
    {
        uint32_t ok = 0;
        if (lane == 0) ok = lzma_rc_start(d, io) ? 1u : 0u;
        return __shfl(ok, 0, 64) != 0;
    }
    __device__ int run(LzmaDec& d, uint16_t* probs, Lzma2CheckDevIO& io, uint64_t& pos, uint64_t& dpos, uint64_t chunk_end, uint32_t* dist,
                       uint32_t* len)
    {
        int r = kRunError;
        if (lane == 0) {
            NoOps ops;
            r = lzma_run(d, probs, io, pos, dpos, chunk_end, dist, len, ops);
        }
        r = __shfl(r, 0, 64);
        pos = shfl0_u64(pos);
        dpos = shfl0_u64(dpos);
        *dist = __shfl(*dist, 0, 64);
        *len = __shfl(*len, 0, 64);
        return r;
    }
    // the first i with a[i] != b[i], or n (n and the pointers are the same on all lanes, and so is the answer)
    __device__ uint32_t differ(const uint8_t* a, const uint8_t* b, uint32_t n)
    {
        for (uint32_t base = 0; base < n; base += 64) {
            const uint32_t i = base + lane;
            const bool bad = i < n && a[i] != b[i];
            const unsigned long long m = __ballot(bad);
            if (m) return base + (uint32_t)__builtin_ctzll(m);
        }
        return n;
    }
};

// chunk c0 + blockIdx.x of the nch the stream has
__global__ __launch_bounds__(64) void lzma2_check_kernel(const uint8_t* __restrict__ in, uint64_t n_in, uint64_t bsize,
                                                         const uint8_t* __restrict__ z, uint64_t n_z, const uint64_t* __restrict__ z_beg,
                                                         const uint64_t* __restrict__ z_end, uint32_t c0, uint32_t nch, Lzma2Verdict* verdicts)
{
    __shared__ uint16_t probs[kLzCheckProbs];
    const uint32_t c = c0 + blockIdx.x;
    if (c >= nch) return;
    const uint64_t zb = z_beg[c], ze = z_end[c];
    Lzma2CheckDevIO io;
    io.z = z;
    io.in = in;
    io.ip = io.iend = 0;
    io.diff_at = 0;
    io.ov = io.diff = false;
    io.lim = ze;
    io.buf = make_uint4(0, 0, 0, 0);
    io.buf_at = ~0ull - 32;
    Lzma2CheckWaveWalk w{threadIdx.x};
    const Lzma2Verdict v = lzma2_check_walk(io, w, in, n_in, bsize, n_z, zb, ze, c, probs);
    if (threadIdx.x == 0) verdicts[c] = v;
}

} // namespace

hipError_t launch_lzma2_check(const uint8_t* d_in, uint64_t n_in, uint64_t bsize, const uint8_t* d_z, uint64_t n_z, const uint64_t* d_z_beg,
                              const uint64_t* d_z_end, uint32_t c0, uint32_t count, uint32_t nch, Lzma2Verdict* d_verdicts, hipStream_t s)
{
    if (count == 0) return hipSuccess;
    if (count > kLzCheckLaunchChunks || c0 > nch || count > nch - c0) return hipErrorInvalidValue;
    if (bsize == 0 || bsize % kLzCheckChunk != 0 || bsize > 0xffffffffu || (uint64_t)nch * kLzCheckChunk < n_in ||
        (nch && (uint64_t)(nch - 1) * kLzCheckChunk >= n_in))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(lzma2_check_kernel, dim3(count), dim3(64), 0, s, d_in, n_in, bsize, d_z, n_z, d_z_beg, d_z_end, c0, nch, d_verdicts);
    return hipGetLastError();
}

} // namespace snaphash
