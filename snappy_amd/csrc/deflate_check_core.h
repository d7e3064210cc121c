// deflate_check_core.h -- the build side's self-check: does a stretch of DEFLATE blocks decode to exactly
// the bytes it was made from?  Shared by deflate_check_kernel (deflate_check_kernels.hip), a host harness in tests/ and a
// sanitizer program, the way inflate_core.h serves the decoder: one routine, compiled for host and device.
//
// The compressor cuts the staged stream into chunks of kDfCheckChunk bytes and ends every chunk's blocks on a byte
// boundary (an empty stored block, or the chunk is stored), so chunk c of the stream `in` owns one stretch z[0..zn) of the
// compressed bytes.  deflate_check_chunk walks the stretch like inflate_run, but WRITES NOTHING: a literal is compared
// with the staged byte it stands for, a match (length, distance) with the staged stream itself -- in[p .. p+len) against
// in[p-dist .. p-dist+len), which is what a decoder would copy if everything before p decoded right, and everything
// before p has been compared already.  A distance may reach in front of the chunk (any valid RFC 1951 sequence is
// accepted, not only the producer's, whose chunks are self-contained), but not beyond min(32768, bytes of `in` in front
// of p).
//
// A chunk is accepted when its blocks produce exactly its bytes AND end exactly at the end of its stretch:
//   not the member's last chunk:  no block has BFINAL set, and a block ends on the bit zn * 8 -- the byte boundary after
//                                 the empty stored block, or the end of a stored chunk;
//   the member's last chunk:      (final) the block with BFINAL set is the last, and the byte after it is z + zn.
// Every path is bounded as in inflate_run: bytes past zn read as zeros and end the walk (every block spends at least three
// bits, every symbol at least one, and the walk stops once it has consumed more than zn * 8 bits); `in` is read only inside
// [0, n_in), the stretch only inside [0, zn).
#pragma once
#include <stdint.h>

#include "inflate_core.h"

namespace snaphash {

constexpr uint32_t kDfCheckChunk = 65536; // input bytes per chunk: the compressor's (deflate_core.h kDfChunk)

enum : uint32_t {
    kDfCheckOk = 0,
    kDfCheckLiteral = 1,  // a literal (or a stored byte) is not the staged byte at `offset`
    kDfCheckMatch = 2,    // a match's copy differs from the staged stream at `offset`
    kDfCheckDistance = 3, // a distance beyond min(32768, bytes in front of the match at `offset`)
    kDfCheckBad = 4,      // RFC 1951 forbids it (or BFINAL inside a chunk that is not the last); `offset` bytes were good
    kDfCheckLong = 5,     // the blocks go on producing after the chunk's last byte
    kDfCheckShort = 6,    // the blocks end at the stretch's end, `offset` bytes into the chunk
    kDfCheckEnd = 7,      // the blocks do not end at the stretch's end (they run past it, or stop before it)
    kDfCheckTable = 8,    // the chunk's entry of the offset table lies outside the compressed buffer (nothing was read)
};

struct DfCheckVerdict {
    uint32_t status; // kDfCheck*
    uint32_t offset; // within the chunk: the first byte that differs, else how far the walk had come
};

IF_HD bool df_check_distance_ok(uint64_t dist, uint64_t front) { return dist <= (front < kInfWindow ? front : kInfWindow); }

// Chunk [p0, p0 + len) of in[0..n_in) against the stretch z[0..zn).  t: scratch for the Huffman tables (LDS on the GPU).
IF_HD DfCheckVerdict deflate_check_chunk(const uint8_t* in, uint64_t n_in, uint64_t p0, uint32_t len, const uint8_t* z, uint64_t zn,
                                         bool final, InflateTables& t)
{
    const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    const uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    const uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
                                6145, 8193, 12289, 16385, 24577};
    const uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    uint32_t o = 0; // bytes of the chunk compared so far
#define DFC_END(st, at) return DfCheckVerdict{(uint32_t)(st), (uint32_t)(at)}
    if (p0 > n_in || len > n_in - p0 || len > kDfCheckChunk) DFC_END(kDfCheckTable, 0);
    const uint8_t* src = in + p0;
    InfBits b;
    b.in = z;
    b.n = zn;
    b.pos = 0;
    b.buf = 0;
    b.cnt = 0;
    for (;;) {
        ib_fill(b);
        if (!final && ib_consumed(b) == zn * 8) DFC_END(o == len ? kDfCheckOk : kDfCheckShort, o);
        const uint32_t last = ib_take(b, 1), type = ib_take(b, 2);
        if (ib_over(b)) DFC_END(kDfCheckEnd, o);
        if (last && !final) DFC_END(kDfCheckBad, o);
        if (type == 0) {
            ib_take(b, b.cnt & 7); // to the byte boundary
            const uint64_t at = ib_consumed(b) >> 3;
            if (at + 4 > zn) DFC_END(kDfCheckEnd, o);
            const uint32_t n = z[at] | (uint32_t)z[at + 1] << 8, nn = z[at + 2] | (uint32_t)z[at + 3] << 8;
            if (n != (~nn & 0xffffu)) DFC_END(kDfCheckBad, o);
            if (at + 4 + n > zn) DFC_END(kDfCheckEnd, o);
            if (n > len - o) DFC_END(kDfCheckLong, o);
            for (uint32_t i = 0; i < n; ++i)
                if (z[at + 4 + i] != src[o + i]) DFC_END(kDfCheckLiteral, o + i);
            o += n;
            b.pos = at + 4 + n;
            b.buf = 0;
            b.cnt = 0;
        } else {
            if (type == 1) {
                inf_fixed(t);
            } else if (type == 2) {
                if (!inf_dynamic(b, t)) DFC_END(ib_over(b) ? kDfCheckEnd : kDfCheckBad, o);
            } else {
                DFC_END(kDfCheckBad, o);
            }
            for (;;) {
                ib_fill(b);
                const int32_t s = inf_decode(b, t.lit);
                if (ib_over(b)) DFC_END(kDfCheckEnd, o);
                if (s < 0) DFC_END(kDfCheckBad, o);
                if (s < 256) {
                    if (o >= len) DFC_END(kDfCheckLong, o);
                    if (src[o] != (uint8_t)s) DFC_END(kDfCheckLiteral, o);
                    ++o;
                    continue;
                }
                if (s == 256) break;
                if (s > 285) DFC_END(kDfCheckBad, o);
                const uint32_t n = lbase[s - 257] + ib_take(b, lext[s - 257]);
                const int32_t ds = inf_decode(b, t.dist);
                if (ds < 0 || ds > 29) DFC_END(kDfCheckBad, o);
                const uint32_t d = dbase[ds] + ib_take(b, dext[ds]);
                if (ib_over(b)) DFC_END(kDfCheckEnd, o);
                if (n > len - o) DFC_END(kDfCheckLong, o);
                if (!df_check_distance_ok(d, p0 + o)) DFC_END(kDfCheckDistance, o);
                const uint8_t* p = src + o;
                const uint8_t* q = p - d; // >= in: d <= p0 + o
                for (uint32_t i = 0; i < n; ++i)
                    if (p[i] != q[i]) DFC_END(kDfCheckMatch, o + i);
                o += n;
            }
        }
        if (last) { // (final only) the byte after the final block is the stretch's end
            if (o != len) DFC_END(kDfCheckShort, o);
            DFC_END(((ib_consumed(b) + 7) >> 3) == zn ? kDfCheckOk : kDfCheckEnd, o);
        }
    }
#undef DFC_END
}

// Chunk c of a table: where its stretch lies.  z_sizes == nullptr: [z_off[c], z_off[c + 1]); else [z_off[c], z_off[c] + z_sizes[c])
// (the producer's prefix and size tables).  A stretch outside [0, z_total) is kDfCheckTable and nothing is read.
IF_HD DfCheckVerdict deflate_check_entry(const uint8_t* in, uint64_t n_in, const uint8_t* z, uint64_t z_total, const uint64_t* z_off,
                                         const uint32_t* z_sizes, uint32_t c, bool final, InflateTables& t)
{
    const uint64_t p0 = (uint64_t)c * kDfCheckChunk;
    const uint32_t len = p0 >= n_in ? 0u : (uint32_t)(n_in - p0 < kDfCheckChunk ? n_in - p0 : kDfCheckChunk);
    const uint64_t z0 = z_off[c], z1 = z_sizes ? z0 + z_sizes[c] : z_off[c + 1];
    if (z0 > z1 || z1 > z_total) return DfCheckVerdict{kDfCheckTable, 0};
    return deflate_check_chunk(in, n_in, p0 >= n_in ? n_in : p0, len, z + z0, z1 - z0, final, t);
}

} // namespace snaphash
