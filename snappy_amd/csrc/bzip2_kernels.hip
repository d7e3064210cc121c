// bzip2_kernels.hip -- the GPU bzip2 decode of the data.tar.bz2 side.  A bzip2 block needs nothing from any other
// block, so every stage runs blocks side by side:
//   scan     every bit offset of the piece: does the 48-bit block magic start here?  (a candidate block start)
//   symbols  one workgroup per candidate, speculatively: bzip2_core.h's header + Huffman + RUNA/RUNB + MTF decode into
//            the candidate's slot; lane 0 decodes -- the walk through a Huffman stream is one serial chain -- with the
//            tables and selectors in LDS (35 KiB: four workgroups a CU)
//   (host)   links the blocks from the stream header: the next one starts where the last ended; false candidates drop
//            out, a block that fails goes to the host decoder
//   ibwt     1024 lanes a linked block: the byte histogram per wave, a prefix, a stable scatter (a wave ranks equal
//            bytes among its 64 lanes with eight ballots) into the T vector; then the permutation walk from origPtr
//            split at 2048 sampled positions (bzip2_core.h's bz_samples .. bz_sample_write) -- each lane walks from
//            its samples to the next marked position, lane 0 links the pieces of the cycle through origPtr, and the walk
//            runs again writing them at the known offsets.  One walker would take n dependent loads of a 3.6 MB vector;
//            here each takes about n / 2048.  A block that is periodic after RLE1 (u^k) has k cycles: the one through
//            origPtr spells u, and the n-step walk repeats it, so its L bytes are copied on to fill the block
//   rle1     1024 chunks a block: each chunk run from every one of the five entry states of the RLE1 undo, the chunks
//            linked by lane 0, the block sizes prefix-summed on the host, then every chunk writes at its final offset.
// Integer work with data-dependent control flow: no MFMA.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bzip2_core.h"
#include "bzip2_kernels.h"

namespace snaphash {

namespace {

__global__ void __launch_bounds__(256) bz_scan_kernel(const uint8_t* __restrict__ in, uint64_t n, uint64_t* cand, uint32_t* count, uint32_t cap)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint64_t w = 0;
        for (uint32_t k = 0; k < 8; ++k) w = w << 8 | (i + k < n ? in[i + k] : 0);
        for (uint32_t sh = 0; sh < 8; ++sh) {
            if (((w << sh) >> 16) != kBzBlockMagic) continue;
            const uint64_t bit = i * 8 + sh;
            if (bit + 48 > n * 8) continue;
            const uint32_t k = atomicAdd(count, 1u);
            if (k < cap) cand[k] = bit;
        }
    }
}

__global__ void __launch_bounds__(64) bz_symbols_kernel(const uint8_t* __restrict__ in, uint64_t n, const uint64_t* __restrict__ starts,
                                                        uint8_t* slots, BzBlockRes* res)
{
    __shared__ BzTables t;
    if (threadIdx.x != 0) return;
    const uint32_t i = blockIdx.x;
    res[i] = bz_block_symbols(in, n, starts[i], slots + (uint64_t)i * kBzMaxBlock, kBzMaxBlock, nullptr, t);
}

__global__ void __launch_bounds__(1024) bz_ibwt_kernel(uint8_t* slots, uint32_t* tts, BzGpuBlock* blocks)
{
    __shared__ uint32_t hist[16][256];
    __shared__ uint32_t slen[kBzWalkers + 1], snext[kBzWalkers + 1], soff[kBzWalkers + 1];
    __shared__ uint32_t cyc;
    BzGpuBlock& B = blocks[blockIdx.x];
    const uint32_t n = B.n, op = B.orig_ptr;
    if (n == 0 || n > kBzMaxBlock || op >= n) { // (the host links no such block)
        if (threadIdx.x == 0) B.status = kBzBad;
        return;
    }
    uint8_t* bwt = slots + (uint64_t)B.slot * kBzMaxBlock;
    uint32_t* tt = tts + (uint64_t)B.slot * kBzMaxBlock;
    const uint32_t tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    for (uint32_t i = tid; i < 16 * 256; i += 1024) (&hist[0][0])[i] = 0;
    __syncthreads();
    // each wave owns a contiguous sixteenth of the block
    const uint32_t a = (uint32_t)((uint64_t)n * w / 16), e = (uint32_t)((uint64_t)n * (w + 1) / 16);
    for (uint32_t i = a + lane; i < e; i += 64) atomicAdd(&hist[w][bwt[i]], 1u);
    __syncthreads();
    if (tid < 256) {
        uint32_t s = 0;
        for (uint32_t k = 0; k < 16; ++k) s += hist[k][tid];
        slen[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t s = 0;
        for (uint32_t c = 0; c < 256; ++c) {
            const uint32_t v = slen[c];
            slen[c] = s;
            s += v;
        }
    }
    __syncthreads();
    if (tid < 256) { // where each wave's first byte of value tid goes
        uint32_t run = slen[tid];
        for (uint32_t k = 0; k < 16; ++k) {
            const uint32_t v = hist[k][tid];
            hist[k][tid] = run;
            run += v;
        }
    }
    __syncthreads();
    // the stable scatter: 64 positions at a time in order, each lane ranked among the lanes that hold its byte
    for (uint32_t base = a; base < e; base += 64) {
        const uint32_t i = base + lane;
        const bool valid = i < e;
        const uint32_t c = valid ? bwt[i] : 0;
        uint64_t peers = __ballot(valid);
        for (uint32_t b = 0; b < 8; ++b) {
            const bool bit = (c >> b) & 1u;
            const uint64_t m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const uint32_t at = hist[w][c]; // (every lane reads before the group's first lane moves it on)
        if (valid) {
            const uint32_t j = at + (uint32_t)__popcll(peers & ((1ull << lane) - 1));
            if (j < n) tt[j] = i << 8;
            if (lane == (uint32_t)(__ffsll((long long)peers) - 1)) hist[w][c] = at + (uint32_t)__popcll(peers);
        }
    }
    __syncthreads();
    // each position's own byte in the low bits, the sampled positions marked
    const BzSamples g = bz_samples(n, op);
    for (uint32_t j = tid; j < n; j += 1024) tt[j] |= bwt[j] | (bz_is_sample(g, j) ? kBzMark : 0u);
    __syncthreads();
    for (uint32_t s = tid; s < g.nsamp; s += 1024) slen[s] = bz_sample_walk(g, tt, s, &snext[s]);
    __syncthreads();
    if (tid == 0) { // the pieces of the cycle through origPtr, in walk order
        cyc = bz_link_samples(g, slen, snext, soff);
        B.status = cyc ? kBzOk : kBzBad;
    }
    __syncthreads();
    const uint32_t L = cyc;
    if (!L) return;
    for (uint32_t s = tid; s < g.nsamp; s += 1024)
        if (soff[s] != kBzNoPiece) bz_sample_write(g, tt, s, slen[s], bwt + soff[s]);
    if (L == n) return;
    __syncthreads();
    // a shorter cycle (a periodic block): the n steps from origPtr go round it, so its L bytes repeat
    for (uint32_t k = L + tid; k < n; k += 1024) bwt[k] = bwt[k % L];
}

__device__ inline uint32_t chunk_size(uint32_t n) { return max(64u, (n + kBzChunks - 1) / kBzChunks); }

__global__ void __launch_bounds__(1024) bz_rle1_count_kernel(const uint8_t* __restrict__ slots, BzGpuBlock* blocks, uint64_t* chunks)
{
    __shared__ uint32_t clen[kBzChunks][5];
    __shared__ uint8_t cexit[kBzChunks][5];
    BzGpuBlock& B = blocks[blockIdx.x];
    if (B.status != kBzOk) return;
    const uint32_t n = B.n, cs = chunk_size(n), nch = (n + cs - 1) / cs;
    const uint8_t* pre = slots + (uint64_t)B.slot * kBzMaxBlock;
    const uint32_t t = threadIdx.x;
    if (t < nch) {
        const uint32_t a = t * cs, e = min(n, a + cs);
        BzRle1 st[5];
        uint32_t len[5];
        for (uint32_t r = 0; r < 5; ++r) {
            st[r].run = r;
            st[r].last = a ? pre[a - 1] : 0;
            len[r] = 0;
        }
        for (uint32_t i = a; i < e; ++i) {
            const uint8_t v = pre[i];
            for (uint32_t r = 0; r < 5; ++r) {
                bool cnt;
                len[r] += bz_rle1_step(st[r], v, cnt);
            }
        }
        for (uint32_t r = 0; r < 5; ++r) {
            clen[t][r] = len[r];
            cexit[t][r] = (uint8_t)st[r].run;
        }
    }
    __syncthreads();
    if (t == 0) {
        uint64_t off = 0;
        uint32_t r = 0;
        uint64_t* ch = chunks + (uint64_t)B.slot * kBzChunks;
        for (uint32_t k = 0; k < nch; ++k) {
            ch[k] = off << 3 | r;
            off += clen[k][r];
            r = cexit[k][r];
        }
        B.out_len = off;
    }
}

__global__ void __launch_bounds__(1024) bz_rle1_write_kernel(const uint8_t* __restrict__ slots, const BzGpuBlock* __restrict__ blocks,
                                                             const uint64_t* __restrict__ chunks, uint8_t* __restrict__ out)
{
    const BzGpuBlock B = blocks[blockIdx.x];
    if (B.status != kBzOk) return;
    const uint32_t n = B.n, cs = chunk_size(n), nch = (n + cs - 1) / cs;
    const uint32_t t = threadIdx.x;
    if (t >= nch) return;
    const uint8_t* pre = slots + (uint64_t)B.slot * kBzMaxBlock;
    const uint64_t e0 = chunks[(uint64_t)B.slot * kBzChunks + t];
    const uint32_t a = t * cs, e = min(n, a + cs);
    BzRle1 st;
    st.run = (uint32_t)(e0 & 7);
    st.last = a ? pre[a - 1] : 0;
    uint8_t* o = out + B.out_off + (e0 >> 3);
    const uint64_t room = B.out_len - (e0 >> 3);
    uint64_t k = 0;
    for (uint32_t i = a; i < e; ++i) {
        bool cnt;
        const uint8_t v = pre[i];
        const uint32_t m = bz_rle1_step(st, v, cnt);
        if (m > room - k) return; // (cannot happen: the first pass measured these very bytes)
        const uint8_t b = cnt ? (uint8_t)st.last : v;
        for (uint32_t q = 0; q < m; ++q) o[k + q] = b;
        k += m;
    }
}

} // namespace

hipError_t launch_bz_scan(const uint8_t* d_in, uint64_t n, uint64_t* d_cand, uint32_t* d_count, uint32_t cap, hipStream_t s)
{
    if (n < 6) return hipSuccess;
    const uint64_t blocks = std::min<uint64_t>((n + 255) / 256, 8192);
    bz_scan_kernel<<<(uint32_t)blocks, 256, 0, s>>>(d_in, n, d_cand, d_count, cap);
    return hipGetLastError();
}

hipError_t launch_bz_symbols(const uint8_t* d_in, uint64_t n, const uint64_t* d_starts, uint32_t count, uint8_t* d_slots,
                             BzBlockRes* d_res, hipStream_t s)
{
    if (count == 0) return hipSuccess;
    bz_symbols_kernel<<<count, 64, 0, s>>>(d_in, n, d_starts, d_slots, d_res);
    return hipGetLastError();
}

hipError_t launch_bz_ibwt(uint8_t* d_slots, uint32_t* d_tt, BzGpuBlock* d_blocks, uint32_t count, hipStream_t s)
{
    if (count == 0) return hipSuccess;
    bz_ibwt_kernel<<<count, 1024, 0, s>>>(d_slots, d_tt, d_blocks);
    return hipGetLastError();
}

hipError_t launch_bz_rle1_count(const uint8_t* d_slots, BzGpuBlock* d_blocks, uint64_t* d_chunks, uint32_t count, hipStream_t s)
{
    if (count == 0) return hipSuccess;
    bz_rle1_count_kernel<<<count, 1024, 0, s>>>(d_slots, d_blocks, d_chunks);
    return hipGetLastError();
}

hipError_t launch_bz_rle1_write(const uint8_t* d_slots, const BzGpuBlock* d_blocks, const uint64_t* d_chunks, uint32_t count,
                                uint8_t* d_out, hipStream_t s)
{
    if (count == 0) return hipSuccess;
    bz_rle1_write_kernel<<<count, 1024, 0, s>>>(d_slots, d_blocks, d_chunks, d_out);
    return hipGetLastError();
}

} // namespace snaphash
