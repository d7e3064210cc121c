// bz2_check_kernels.hip -- the .bz2 producer's self-check on gfx950: while a slot is being coded the staged
// tar stream and the shifted-together blocks are both in HBM, so whether every block decodes back to its piece is decided
// there, before a byte travels to the host.  bz2_check_core.h holds what host and device share; the steps:
//   symbols  one 64-lane workgroup a block, lane 0 walking (the walk through a Huffman stream is one serial chain), the
//            tables and selectors in LDS (BzTables, 35 KiB: four workgroups a CU of 160 KiB) -- bz_symbols_kernel's shape,
//            with the cap a decoder allows the stream's level and a table entry that is checked before anything is read
//   link     one lane a block: bz2_check_link turns the symbol stage's result into the decoder's BzGpuBlock, or into an
//            early verdict and a block the later kernels skip -- the install side links on the host; here nobody waits
//   (the install side's bz_ibwt_kernel and bz_rle1_count_kernel, as they are)
//   compare  1 024 lanes a block, one RLE1 chunk a lane from the entry state and offset bz_rle1_count_kernel left in
//            d_chunks: bz_rle1_write_kernel's loop with the store replaced by a compare.  Each lane's first difference is
//            its lowest (its positions ascend); a wave takes the minimum over its lanes by six shuffles, its first
//            lane folds that into one LDS word with atomicMin (sixteen atomics a block at most, four bytes of LDS), and
//            lane 0 writes the verdict behind one barrier: the FIRST differing byte, whatever order the lanes finish in.
// Integer work with data-dependent control flow: no MFMA.  Not HBM-bound: symbols is one lane's chain, the rest reads a
// block's 0.9 MB a few times.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bz2_check_core.h"
#include "bz2_check_kernels.h"

namespace snaphash {

namespace {

__global__ void __launch_bounds__(64) bz2_check_symbols_kernel(const uint8_t* __restrict__ z, uint64_t n_z, uint64_t n_in,
                                                               const Bz2CheckJob* __restrict__ jobs, uint32_t cap, uint8_t* slots, BzBlockRes* res)
{
    __shared__ BzTables t;
    if (threadIdx.x != 0) return;
    const uint32_t i = blockIdx.x;
    const Bz2CheckJob j = jobs[i];
    BzBlockRes r;
    if (bz2_check_table_ok(j, n_z, n_in)) r = bz_block_symbols(z, n_z, j.z_beg, slots + (uint64_t)i * kBzMaxBlock, cap, nullptr, t);
    res[i] = r;
}

__global__ void __launch_bounds__(64) bz2_check_link_kernel(const BzBlockRes* __restrict__ res, const Bz2CheckJob* __restrict__ jobs, uint64_t n_z,
                                                            uint64_t n_in, uint32_t level, uint32_t count, BzGpuBlock* blocks, Bz2Verdict* verdicts)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    BzGpuBlock B;
    verdicts[i] = bz2_check_link(res[i], jobs[i], n_z, n_in, level, i, B);
    blocks[i] = B;
}

__global__ void __launch_bounds__(1024) bz2_check_compare_kernel(const uint8_t* __restrict__ slots, const BzGpuBlock* __restrict__ blocks,
                                                                 const uint64_t* __restrict__ chunks, const uint8_t* __restrict__ staged,
                                                                 const Bz2CheckJob* __restrict__ jobs, Bz2Verdict* verdicts)
{
    __shared__ uint32_t first; // the lowest differing offset (a block decodes to fewer than 2^32 bytes)
    const uint32_t t = threadIdx.x;
    if (verdicts[blockIdx.x].status != kBz2CheckPending) return; // an early verdict stands (the same on every lane)
    const BzGpuBlock B = blocks[blockIdx.x];
    if (B.status != kBzOk) { // the inverse BWT's walk broke
        if (t == 0) verdicts[blockIdx.x] = bz2_verdict(kBz2CheckOrigPtr, B.orig_ptr);
        return;
    }
    const Bz2CheckJob j = jobs[blockIdx.x];
    if (t == 0) first = ~0u;
    __syncthreads();
    const uint32_t n = B.n, cs = bz2_check_chunk_size(n), nch = (n + cs - 1) / cs;
    uint32_t mine = ~0u;
    if (t < nch) {
        const uint8_t* pre = slots + (uint64_t)B.slot * kBzMaxBlock;
        const uint64_t e0 = chunks[(uint64_t)B.slot * kBzChunks + t];
        const uint32_t a = t * cs, e = min(n, a + cs);
        BzRle1 st;
        st.run = (uint32_t)(e0 & 7);
        st.last = a ? pre[a - 1] : 0;
        const uint64_t d = bz2_check_compare(st, pre, a, e, e0 >> 3, staged + j.in_off, j.in_len);
        if (d != ~0ull) mine = (uint32_t)d;
    }
    for (uint32_t s = 32; s > 0; s >>= 1) mine = min(mine, (uint32_t)__shfl_xor((int)mine, (int)s, 64));
    if ((t & 63) == 0 && mine != ~0u) atomicMin(&first, mine);
    __syncthreads();
    if (t == 0) verdicts[blockIdx.x] = bz2_check_final(first == ~0u ? ~0ull : first, B.out_len, j.in_len);
}

} // namespace

hipError_t launch_bz2_check_symbols(const uint8_t* d_z, uint64_t n_z, uint64_t n_in, const Bz2CheckJob* d_jobs, uint32_t level, uint32_t count,
                                    uint8_t* d_slots, BzBlockRes* d_res, hipStream_t s)
{
    if (count == 0) return hipSuccess;
    if (level < 1 || level > 9) return hipErrorInvalidValue;
    bz2_check_symbols_kernel<<<count, 64, 0, s>>>(d_z, n_z, n_in, d_jobs, bz2_check_cap(level), d_slots, d_res);
    return hipGetLastError();
}

hipError_t launch_bz2_check_link(const BzBlockRes* d_res, const Bz2CheckJob* d_jobs, uint64_t n_z, uint64_t n_in, uint32_t level, uint32_t count,
                                 BzGpuBlock* d_blocks, Bz2Verdict* d_verdicts, hipStream_t s)
{
    if (count == 0) return hipSuccess;
    bz2_check_link_kernel<<<(count + 63) / 64, 64, 0, s>>>(d_res, d_jobs, n_z, n_in, level, count, d_blocks, d_verdicts);
    return hipGetLastError();
}

hipError_t launch_bz2_check_compare(const uint8_t* d_slots, const BzGpuBlock* d_blocks, const uint64_t* d_chunks, const uint8_t* d_in,
                                    const Bz2CheckJob* d_jobs, uint32_t count, Bz2Verdict* d_verdicts, hipStream_t s)
{
    if (count == 0) return hipSuccess;
    bz2_check_compare_kernel<<<count, 1024, 0, s>>>(d_slots, d_blocks, d_chunks, d_in, d_jobs, d_verdicts);
    return hipGetLastError();
}

} // namespace snaphash
