// xz_kernels.hip -- the LZMA2 Blocks of a .xz file decoded side by side on gfx950, a 64-lane workgroup a Block.
//
// Inside a Block LZMA is one serial chain (the probabilities carry from symbol to symbol and from chunk to chunk), so a
// Block is one lane's work: lane 0 runs the range decoder of xz_core.h with the probabilities (at most 14 134 entries,
// 28 268 bytes: five workgroups a CU) in LDS, the previous byte and the rep distances in registers and the compressed
// bytes prefetched sixteen at a time.  What the wave adds is width where there is some: the probabilities are reset by
// all lanes, and match bodies (up to 273 bytes) and uncompressed chunks are copied by all lanes -- for a distance below
// the length the source repeats, out[pos + i] = out[pos - dist + i % dist], which only reads bytes written before the
// body.  The Block's output at its final offset is the dictionary.
//
// Bytes stored by one lane are read by another (lane 0 reads the match byte of the literal after a match out of a body
// the wave copied; the wave copies literals lane 0 stored).  The compiler sees no dependence across lanes, so both sides of
// every wave copy carry __syncthreads(): a workgroup-scope fence that also waits for the stores (the workgroup is one
// wave, the barrier itself costs nothing).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "xz_core.h"
#include "xz_kernels.h"

namespace snaphash {

namespace {

struct XzDevIO {
    const uint8_t* in; // the Block's LZMA2 data
    uint64_t lim;      // its length: no load goes past it
    uint64_t ip, iend; // the chunk's compressed bytes
    uint8_t* out;      // the Block's output
    uint4 buf;         // in[buf_at .. buf_at + 16)
    uint64_t buf_at;
    bool ov;
    __device__ uint32_t in_at(uint64_t p) const { return in[p]; }
    __device__ uint32_t next()
    {
        if (ip >= iend) {
            ov = true;
            return 0;
        }
        const uint64_t i = ip++;
        uint64_t k = i - buf_at;
        if (k >= 16) {
            if ((((uintptr_t)(in + i)) & 15) != 0 || lim - i < 16) return in[i];
            buf = *(const uint4*)(in + i);
            buf_at = i;
            k = 0;
        }
        const uint32_t w = k < 8 ? (k < 4 ? buf.x : buf.y) : (k < 12 ? buf.z : buf.w);
        return (w >> (8 * ((uint32_t)k & 3))) & 0xff;
    }
    __device__ bool over() const { return ov; }
    __device__ uint32_t out_at(uint64_t p) const { return out[p]; }
    __device__ void put(uint64_t p, uint32_t b) { out[p] = (uint8_t)b; }
};

__device__ inline uint64_t shfl0_u64(uint64_t v)
{
    const uint32_t lo = __shfl((uint32_t)v, 0, 64), hi = __shfl((uint32_t)(v >> 32), 0, 64);
    return (uint64_t)hi << 32 | lo;
}

__global__ __launch_bounds__(kXzWave) void lzma2_blocks_kernel(const uint8_t* in, uint8_t* out, XzGpuBlock* blk, uint32_t nb)
{
    __shared__ uint16_t probs[kLzmaProbsMax];
    const uint32_t lane = threadIdx.x;
    for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const XzGpuBlock B = blk[b];
        XzDevIO io;
        io.in = in + B.in_off;
        io.lim = B.in_len;
        io.out = out + B.out_off;
        io.ip = io.iend = 0;
        io.buf = make_uint4(0, 0, 0, 0);
        io.buf_at = ~0ull - 32;
        io.ov = false;
        LzmaDec d{};
        d.dict_size = B.dict_size;
        NoOps ops;
        uint64_t at = 0, pos = 0, dpos = 0; // the same on every lane
        bool need_dict = true, need_props = true;
        uint32_t status = kXzBad;
        for (;;) {
            Lzma2Chunk c;
            if (lzma2_chunk_header(io, at, B.in_len, need_dict, need_props, c)) break;
            if (c.kind == 0) {
                if (at + 1 == B.in_len && pos == B.out_len) status = kXzOk;
                break;
            }
            at += c.hdr;
            if (c.csize > B.in_len - at || c.usize > B.out_len - pos) break;
            if (c.dict_reset) {
                dpos = 0;
                need_props = true;
            }
            need_dict = false;
            if (c.kind == 1) {
                for (uint32_t i = lane; i < c.usize; i += kXzWave) io.out[pos + i] = io.in[at + i];
                d.prev = io.in[at + c.usize - 1];
                pos += c.usize;
                dpos += c.usize;
                at += c.csize;
                __syncthreads();
                continue;
            }
            if (c.new_props) {
                d.lc = c.lc;
                d.lp_mask = (1u << c.lp) - 1;
                d.pb_mask = (1u << c.pb) - 1;
                need_props = false;
            }
            if (c.state_reset) {
                lzma_reset_state(d);
                const uint32_t np = lzma_probs_count(d.lc, (uint32_t)__builtin_popcount(d.lp_mask));
                for (uint32_t i = lane; i < np; i += kXzWave) probs[i] = kLzmaProbInit;
                __syncthreads();
            }
            if (dpos == 0) d.prev = 0;
            const uint64_t chunk_end = pos + c.usize;
            int r = kRunChunkEnd;
            if (lane == 0) {
                io.ip = at;
                io.iend = at + c.csize;
                io.ov = false;
                if (!lzma_rc_start(d, io)) r = kRunError;
            }
            for (;;) {
                uint32_t dist = 0, len = 0;
                if (lane == 0 && r != kRunError) r = lzma_run(d, probs, io, pos, dpos, chunk_end, &dist, &len, ops);
                r = __shfl(r, 0, 64);
                if (r != kRunMatch) break;
                pos = shfl0_u64(pos);
                dpos = shfl0_u64(dpos);
                dist = __shfl(dist, 0, 64);
                len = __shfl(len, 0, 64);
                __syncthreads(); // lane 0's literals are in place for every lane
                const uint32_t last = xz_copy_lane(io.out, pos, dist, len, lane);
                d.prev = __shfl(last, (len - 1) & (kXzWave - 1), 64);
                pos += len;
                dpos += len;
                __syncthreads(); // and the body for lane 0
            }
            pos = shfl0_u64(pos);
            dpos = shfl0_u64(dpos);
            uint32_t bad = r == kRunError || io.ov || io.ip != io.iend || d.code != 0;
            bad = __shfl(bad, 0, 64);
            if (bad) break;
            at += c.csize;
            __syncthreads(); // lane 0's last literals, for an uncompressed chunk's or the next chunk's copies
        }
        if (lane == 0) blk[b].status = status;
        __syncthreads(); // the next Block resets the probabilities
    }
}

} // namespace

hipError_t launch_lzma2_blocks(const uint8_t* d_in, uint8_t* d_out, XzGpuBlock* d_blk, uint32_t nb, hipStream_t s)
{
    if (nb == 0) return hipSuccess;
    const uint32_t grid = nb < 1280 ? nb : 1280; // 256 CUs x 5 workgroups (28 KiB of LDS each)
    hipLaunchKernelGGL(lzma2_blocks_kernel, dim3(grid), dim3(kXzWave), 0, s, d_in, d_out, d_blk, nb);
    return hipGetLastError();
}

} // namespace snaphash
