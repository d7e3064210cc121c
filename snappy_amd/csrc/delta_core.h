// delta_core.h -- the .xz format's Delta filter (id 0x03), shared by the GPU kernels (delta_kernels.hip) and a host harness
// in tests/, the way bcj_core.h serves its users.  Written from the .xz file format specification (5.3.1) and held byte for
// byte against liblzma 5.2.5.
//
// With a distance d in 1 .. 256 (the one property byte is d - 1) and bytes modulo 256:
//   encode  out[i] = in[i] - in[i - d]          decode  out[i] = in[i] + out[i - d]
// Bytes in front of the Block are 0; nothing is carried from Block to Block.
//
// Decode is a running sum down each COLUMN, the positions of one residue modulo d, through the whole Block.  The kernels
// cut a Block into tiles of kDeltaTile bytes, and a tile's answer is its own running sums plus, a column, the sum of
// everything in front of the tile: the CARRY.  Columns are counted by the position in the Block, so a tile's first byte is
// column (tile's first position) % d, which moves from tile to tile whenever d does not divide the tile.  Three passes, none of
// which reads what another workgroup of the same pass writes:
//   sums    a tile's column sums, d bytes a tile (delta_lane_sum, delta_tile_total)
//   carry   a range's tiles in order, a lane a column: each tile's sums become the sum of the tiles in front (delta_carry_column)
//   apply   a tile's running sums seeded with its carry, in place (delta_lane_sum, delta_lane_seed, delta_lane_apply)
// Inside a tile the kDeltaLanes lanes are laid out as G = kDeltaLanes / d row groups of d columns: lane g * d + c takes
// column c of the rows of group g (a row: the d positions r * d .. r * d + d - 1 of the Block; a tile's first and last row
// may be partial).  The lanes' sums are scanned over g, and each lane walks its rows.  d = 256: a lane a column and 256
// rows; d = 1: a lane a stretch of 256 bytes.
//
// Encode reads in[i - d], which for a tile's first d bytes lies in the tile in front, where another workgroup writes.  So
// a first pass saves every tile's last kDeltaTail bytes (delta_tail_byte reads them back), and the second one encodes a
// tile from its end to its start, a slab of lanes x kDeltaSlab bytes at a time: every byte of the slab and its byte in front are
// read before any is written.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DELTA_HD __host__ __device__ inline
#else
#define DELTA_HD inline
#endif

namespace snaphash {

constexpr uint32_t kDeltaMaxDist = 256;  // the format's largest distance
constexpr uint32_t kDeltaLanes = 256;    // a workgroup
constexpr uint32_t kDeltaTile = 65536;   // bytes of a range a workgroup takes
constexpr uint32_t kDeltaTail = 256;     // bytes of a tile's end the encoder saves: kDeltaMaxDist
constexpr uint32_t kDeltaSlab = 16;      // bytes a lane holds at a time in the encoder

DELTA_HD bool delta_dist_valid(uint32_t d) { return d >= 1 && d <= kDeltaMaxDist; }

// ---- a whole Block on one thread, in place ---------------------------------------------------------------------------------
DELTA_HD void delta_block(bool encode, uint8_t* b, uint64_t len, uint32_t d)
{
    if (encode) {
        for (uint64_t i = len; i-- > d;) b[i] = (uint8_t)(b[i] - b[i - d]); // from the end: b[i - d] is still the input's
    } else {
        for (uint64_t i = d; i < len; ++i) b[i] = (uint8_t)(b[i] + b[i - d]);
    }
}

// ---- decode, a tile [s, e) of the Block (0 <= s < e <= len), a lane at a time -------------------------------------------------

// The rows [ra, rb) and the column c that `lane` of `lanes` takes; lanes behind the last whole group take nothing (ra == rb).
struct DeltaLane {
    uint64_t ra, rb;
    uint32_t c;
};
DELTA_HD DeltaLane delta_lane(uint64_t s, uint64_t e, uint32_t d, uint32_t lanes, uint32_t lane)
{
    const uint32_t groups = lanes / d, g = lane / d;
    const uint64_t r0 = s / d, r1 = (e - 1) / d + 1;       // the tile's rows, the partial ones included
    const uint64_t per = (r1 - r0 + groups - 1) / groups;  // rows a group
    DeltaLane L;
    L.c = lane % d;
    L.ra = g < groups && r0 + g * per < r1 ? r0 + g * per : r1;
    L.rb = L.ra + per < r1 ? L.ra + per : r1;
    return L;
}
// the sum of the lane's bytes
DELTA_HD uint8_t delta_lane_sum(const uint8_t* b, uint64_t s, uint64_t e, uint32_t d, DeltaLane L)
{
    uint32_t sum = 0;
    for (uint64_t r = L.ra; r < L.rb; ++r) {
        const uint64_t i = r * d + L.c;
        if (i >= s && i < e) sum += b[i];
    }
    return (uint8_t)sum;
}
// what the lane's running sum starts from: the column's carry into the tile and the sums of the groups in front of the lane's
// (part[lane]: every lane's delta_lane_sum)
DELTA_HD uint8_t delta_lane_seed(const uint8_t* part, uint32_t d, uint32_t lane, uint8_t carry)
{
    uint32_t sum = carry;
    for (uint32_t q = lane % d; q < lane; q += d) sum += part[q];
    return (uint8_t)sum;
}
// the column's sum over the whole tile, c < d (the lanes behind the last whole group hold 0)
DELTA_HD uint8_t delta_tile_total(const uint8_t* part, uint32_t d, uint32_t lanes, uint32_t c)
{
    uint32_t sum = 0;
    for (uint32_t g = 0; g < lanes / d; ++g) sum += part[g * d + c];
    return (uint8_t)sum;
}
// the lane's rows, in place
DELTA_HD void delta_lane_apply(uint8_t* b, uint64_t s, uint64_t e, uint32_t d, DeltaLane L, uint8_t seed)
{
    uint32_t run = seed;
    for (uint64_t r = L.ra; r < L.rb; ++r) {
        const uint64_t i = r * d + L.c;
        if (i >= s && i < e) {
            run += b[i];
            b[i] = (uint8_t)run;
        }
    }
}
// column c of a range of nt tiles: sums[t * stride + c], each tile's column sum, becomes the sum of the tiles in front
DELTA_HD void delta_carry_column(uint8_t* sums, uint64_t nt, uint32_t stride, uint32_t c)
{
    uint32_t run = 0;
    for (uint64_t t = 0; t < nt; ++t) {
        const uint32_t v = sums[t * stride + c];
        sums[t * stride + c] = (uint8_t)run;
        run += v;
    }
}

// ---- encode ---------------------------------------------------------------------------------------------------------------------
// byte k of the tail a tile that ends at e leaves for the tile behind it: the kDeltaTail bytes in front of e, as they were
// (0 in front of the Block, which only a tile shorter than kDeltaTail can reach: the host model's)
DELTA_HD uint8_t delta_tail_byte(const uint8_t* b, uint64_t e, uint32_t k) { return e + k >= kDeltaTail ? b[e + k - kDeltaTail] : 0; }
// in[i - d] for a position i of the tile that begins at s: 0 in front of the Block, the saved tail of the tile in front
// (its last kDeltaTail bytes, as they were) in front of s, the tile's own byte otherwise
DELTA_HD uint8_t delta_byte_in_front(const uint8_t* b, uint64_t i, uint32_t d, uint64_t s, const uint8_t* tail_in_front)
{
    if (i < d) return 0;
    const uint64_t j = i - d;
    return j >= s ? b[j] : tail_in_front[kDeltaTail - (s - j)];
}

} // namespace snaphash
