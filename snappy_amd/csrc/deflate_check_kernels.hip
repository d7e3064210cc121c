// deflate_check_kernels.hip -- the build side's self-check on the GPU: while a slot is being compressed the
// staged tar stream and the compacted compressed bytes are both in HBM, so whether the one decodes back to the other is
// decided there, before a byte travels to the host.  deflate_check_core.h holds the walk; here one wave takes one 64 KiB
// chunk, as in the inflate kernel: the walk through a Huffman stream is one serial chain, so lane 0 runs it with its tables
// in LDS (3.9 KB a wave: 32 waves a CU walk side by side), comparisons included -- the verdict is then the host walker's bit
// for bit, whichever byte differs first.  Nothing is written but the chunk's verdict; no holes, no fill pass, no output.
// Integer work with data-dependent control flow: no MFMA.  Not HBM-bound: a chunk is one lane's serial chain.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "deflate_check_core.h"
#include "deflate_check_kernels.h"

namespace snaphash {

namespace {

// chunk chunk0 + blockIdx.x of the nchunks the stream of n_in bytes has; its stretch by deflate_check_entry's rule
__global__ void __launch_bounds__(64) deflate_check_kernel(const uint8_t* __restrict__ in, uint64_t n_in, const uint8_t* __restrict__ z,
                                                           uint64_t z_total, const uint64_t* __restrict__ z_off,
                                                           const uint32_t* __restrict__ z_sizes, uint32_t chunk0, uint32_t nchunks,
                                                           uint32_t last_is_final, DfCheckVerdict* verdicts)
{
    __shared__ InflateTables t;
    if (threadIdx.x != 0) return;
    const uint32_t c = chunk0 + blockIdx.x;
    if (c >= nchunks) return;
    verdicts[c] = deflate_check_entry(in, n_in, z, z_total, z_off, z_sizes, c, last_is_final && c + 1 == nchunks, t);
}

} // namespace

hipError_t launch_deflate_check(const uint8_t* d_in, uint64_t n_in, const uint8_t* d_z, uint64_t z_total, const uint64_t* d_z_off,
                                const uint32_t* d_z_sizes, uint32_t chunk0, uint32_t count, uint32_t nchunks, bool last_is_final,
                                DfCheckVerdict* d_verdicts, hipStream_t s)
{
    if (count == 0) return hipSuccess;
    if (chunk0 > nchunks || count > nchunks - chunk0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(deflate_check_kernel, dim3(count), dim3(64), 0, s, d_in, n_in, d_z, z_total, d_z_off, d_z_sizes, chunk0, nchunks,
                       last_is_final ? 1u : 0u, d_verdicts);
    return hipGetLastError();
}

} // namespace snaphash
