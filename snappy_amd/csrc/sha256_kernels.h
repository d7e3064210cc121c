// sha256_kernels.h -- launcher of the SHA-256 of byte ranges resident in HBM (sha256_kernels.hip).  Internal.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "sha256_core.h"

namespace snaphash {

// Range k of a launch: d_base[off .. off + len), any byte alignment, any length below kSha256RangeMax; its digest goes to
// d_digests + 32 * idx.  A wave takes 64 consecutive entries and runs until the longest of them ends, so the caller
// sorts the entries by sha256_blocks(len), the longest first (sha256_ranges_dev, snaphash_api.cpp).
struct Sha256Range {
    uint64_t off, len;
    uint32_t idx, reserved;
};
constexpr uint64_t kSha256RangeMax = 1ull << 35; // (a range's aligned words and blocks count in 32 bits)

// d_digests: 16-byte aligned, 32 bytes a range, nothing else is written
hipError_t launch_sha256_ranges(const uint8_t* d_base, const Sha256Range* d_ranges, uint32_t n, uint8_t* d_digests, hipStream_t s);

} // namespace snaphash
