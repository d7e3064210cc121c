// crc_kernels.h -- launchers of the CRC-32 of byte ranges resident in HBM (crc_kernels.hip).  Internal.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "crc_core.h"

namespace snaphash {

// Range i is d_base[d_offs[i] .. + d_lens[i]): any byte alignment, any length.  d_tile0 (n + 1 entries) is the prefix sum
// of crc_tiles_of(len): tile_total = d_tile0[n] pairs of (range, tile), one workgroup each in a grid-stride loop, leave
// one raw remainder each in d_partial[0 .. tile_total); launch_crc_fold then shifts every tile's remainder to its place,
// xors them per range (no order is depended on) and writes the n finished CRCs to d_crcs.  kind: kCrcGzip / kCrcBzip2.
hipError_t launch_crc_ranges(int kind, const uint8_t* d_base, const uint64_t* d_offs, const uint64_t* d_lens, const uint32_t* d_tile0,
                             uint32_t n, uint32_t tile_total, uint32_t* d_partial, hipStream_t s);
hipError_t launch_crc_fold(int kind, const uint64_t* d_lens, const uint32_t* d_tile0, uint32_t n, const uint32_t* d_partial,
                           uint32_t* d_crcs, hipStream_t s);

// The same for CRC-64/XZ (the .xz container's Check id 4): 64-bit remainders in d_partial and d_crcs.
hipError_t launch_crc64_ranges(const uint8_t* d_base, const uint64_t* d_offs, const uint64_t* d_lens, const uint32_t* d_tile0, uint32_t n,
                               uint32_t tile_total, uint64_t* d_partial, hipStream_t s);
hipError_t launch_crc64_fold(const uint64_t* d_lens, const uint32_t* d_tile0, uint32_t n, const uint64_t* d_partial, uint64_t* d_crcs,
                             hipStream_t s);

} // namespace snaphash
