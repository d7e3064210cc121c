// Host harness for tests/test_crc_host.py: snappy_amd/csrc/crc_core.h compiled for the CPU -- the same routines the CRC
// kernels run (crc_kernels.hip), and the kernels' cut of a range into tiles and lane slices run serially.
#include <stddef.h>
#include <stdint.h>

#include "../snappy_amd/csrc/crc_core.h"

using namespace snaphash;

namespace {

template <int KIND> struct Ctx {
    uint32_t tab[8][256];
    CrcPowTable pw;
    Ctx()
    {
        crc_tables<KIND>(tab);
        crc_pow_table<KIND>(pw);
    }
};
template <int KIND> const Ctx<KIND>& ctx()
{
    static const Ctx<KIND> c;
    return c;
}

template <int KIND> uint32_t whole(const uint8_t* p, uint64_t n)
{
    const Ctx<KIND>& c = ctx<KIND>();
    return crc_finish<KIND>(c.pw, crc_raw_update<KIND>(c.tab, 0, p, n), n);
}

// as crc_ranges_kernel and crc_fold_kernel: every lane's slice, shifted by its constant, xor'ed per tile; every tile's
// remainder shifted by its constant, xor'ed per range; the init and final xor for the length
template <int KIND> uint32_t tiled(const uint8_t* p, uint64_t n)
{
    const Ctx<KIND>& c = ctx<KIND>();
    uint32_t acc = 0;
    const uint64_t nt = crc_tiles_of(n);
    for (uint64_t k = 0; k < nt; ++k) {
        uint32_t tile = 0;
        for (uint32_t lane = 0; lane < kCrcLanes; ++lane) {
            uint64_t lo, hi;
            crc_lane_slice(n, k, lane, &lo, &hi);
            if (hi > lo) tile ^= crc_mul<KIND>(crc_raw_update<KIND>(c.tab, 0, p + lo, hi - lo), crc_lane_shift<KIND>(c.pw, lane));
        }
        acc ^= crc_mul<KIND>(tile, crc_tile_shift<KIND>(c.pw, k));
    }
    return crc_finish<KIND>(c.pw, acc, n);
}

} // namespace

extern "C" {

uint32_t ch_crc(int kind, const uint8_t* p, uint64_t n) { return kind == kCrcGzip ? whole<kCrcGzip>(p, n) : whole<kCrcBzip2>(p, n); }
uint32_t ch_tiled(int kind, const uint8_t* p, uint64_t n) { return kind == kCrcGzip ? tiled<kCrcGzip>(p, n) : tiled<kCrcBzip2>(p, n); }
uint32_t ch_combine(int kind, uint32_t a, uint32_t b, uint64_t len_b)
{
    return kind == kCrcGzip ? crc_combine<kCrcGzip>(ctx<kCrcGzip>().pw, a, b, len_b) : crc_combine<kCrcBzip2>(ctx<kCrcBzip2>().pw, a, b, len_b);
}
// the bytes a lane covers, so that the test can check the cut itself: every byte of the range exactly once, in order
void ch_slice(uint64_t len, uint64_t k, uint32_t lane, uint64_t* lo, uint64_t* hi) { crc_lane_slice(len, k, lane, lo, hi); }
uint64_t ch_tiles(uint64_t len) { return crc_tiles_of(len); }
uint32_t ch_tile_bytes(void) { return kCrcTile; }
uint32_t ch_slice_bytes(void) { return kCrcSlice; }

} // extern "C"
