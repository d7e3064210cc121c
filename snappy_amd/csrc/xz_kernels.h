// xz_kernels.h -- launcher of the LZMA2 Block decoder for gfx950 (xz_kernels.hip).  Internal.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "xz_core.h"

namespace snaphash {

// A Block whose uncompressed size is larger goes to a host thread even under SNAPHASH_FLAG_GPU_ONLY: one lane walks a
// Block's whole chain, and a launch nobody can tell from a hang has no place on a shared machine.  A quick pass of
// tools/unxz_bench.py saw one lane do 1.3-3.6 MB/s: the bench's 1 MiB Blocks are launches of 0.3-0.8 s,
// a Block at this cap can take about three seconds.  The full-size run that is to settle the value has not been made.
constexpr uint64_t kXzGpuBlockMax = 4ull << 20;

struct XzGpuBlock {
    uint64_t in_off, in_len;   // the LZMA2 data in d_in
    uint64_t out_off, out_len; // where the Block's bytes go in d_out
    uint32_t dict_size;
    uint32_t status;           // out: kXzOk / kXzBad
};

// One 64-lane workgroup per Block (grid-stride over nb): the probabilities in LDS, the range decoder on lane 0, match
// bodies and uncompressed chunks copied by the whole wave.  Nothing outside a Block's [in_off, in_off + in_len) is read
// and nothing outside its [out_off, out_off + out_len) is written.
hipError_t launch_lzma2_blocks(const uint8_t* d_in, uint8_t* d_out, XzGpuBlock* d_blk, uint32_t nb, hipStream_t s);

} // namespace snaphash
