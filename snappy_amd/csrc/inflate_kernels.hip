// inflate_kernels.hip -- the GPU inflate of the install side: the inverse of the block-parallel
// DEFLATE kernel.  The producer ends every 64 KiB chunk on a byte boundary (an empty stored block, or the chunk is
// stored), and pigz / gzip --rsyncable / zlib's Z_SYNC_FLUSH do the same; from such a point on the stream decodes
// without what came before, except for back-references in front of it.  So:
//   scan     every byte: can a non-final stored block end here?  (a candidate segment start)
//   decode   one wave per candidate, speculatively: inflate_core.h's routine in hole mode into a slot of uint16 symbols
//            (a reference in front of the segment is a hole: kInfHole + distance); lane 0 decodes -- the walk through a
//            Huffman stream is one serial chain -- with its tables in LDS, so that 32 waves per CU decode side by side
//   (host)   links the segments from the stream start: the next one starts where the last ended; false candidates drop
//            out, a gap / overflow / failure ends the piece there and goes to the host decoder
//   fill     a hole takes the byte it names from the segment before (or the 32 KiB window in front of the piece):
//            one pass over all segments at once, which leaves the holes whose byte is a hole itself (a match inside a
//            segment that copies a hole makes another one further on: chains that run through every segment of text),
//            then the segments that still hold holes one launch after another, in order -- each one's bytes before it
//            are final by then
//   concat   the symbols as bytes at their prefix-sum offsets.
// Block mode (SNAPHASH_FLAG_SPLIT_BLOCKS) cuts a stream without flush points at its block boundaries instead:
//   block scan  every BIT offset: does a dynamic-Huffman block header that inflate_core.h's inf_dynamic accepts start
//               here?  (inf_dynamic_ok; the stored-block scan above runs beside it)
//   decode      the same kernel from bit starts, stopping at the first block end past kInflateBlockMinOut symbols
//   fill, concat as above, with the block slots' size.
// Integer work with data-dependent control flow: no MFMA.  Not HBM-bound: a segment's decode is one lane's serial chain.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "inflate_core.h"
#include "inflate_kernels.h"

namespace snaphash {

namespace {

__global__ void __launch_bounds__(256) inflate_scan_kernel(const uint8_t* __restrict__ in, uint64_t n, uint32_t* cand, uint32_t* count, uint32_t cap)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j + 4 <= n; j += stride) {
        const uint32_t len = in[j] | (uint32_t)in[j + 1] << 8, nlen = in[j + 2] | (uint32_t)in[j + 3] << 8;
        if (len != (~nlen & 0xffffu)) continue;
        if (len != 0 && (j == 0 || in[j - 1] >= 32)) continue;
        if (j + 4 + len > n) continue;
        const uint32_t k = atomicAdd(count, 1u);
        if (k < cap) cand[k] = (uint32_t)(j + 4 + len);
    }
}

// The block scan.  A workgroup tests the kScanTile * 8 bit offsets of one tile, a wave a quarter of it: each lane one
// byte's 8 offsets at a time.  The tile and a halo that holds any header starting in it (kInfHeaderMaxBits = 2286 bits
// from the last offset, plus the 8 bytes a peek reads: 4095 + 286 + 8 < 4096 + 320) are loaded into LDS once, with
// zeros past the piece's end, so that every offset reads what inf_dynamic_ok on the host reads from in[0..n).
// The cheap half (BTYPE, HLIT, HDIST, a complete precode) runs on every offset in lockstep; the few offsets that pass
// it are compacted into a per-wave LDS queue (ballot + prefix count), and 64 of them at a time take the code-length walk
// one per lane, so that a lone survivor does not hold 63 idle lanes through its walk.  Accepted offsets are appended
// unordered, one atomicAdd per wave and flush.
constexpr uint32_t kScanTile = 4096, kScanHalo = 320;
static_assert(kScanTile - 1 + (kInfHeaderMaxBits + 7) / 8 + 8 < kScanTile + kScanHalo, "the halo must hold a whole header");

__global__ void __launch_bounds__(256) inflate_block_scan_kernel(const uint8_t* __restrict__ in, uint64_t n, uint32_t* cand, uint32_t* count,
                                                                 uint32_t cap)
{
    __shared__ uint32_t tile[(kScanTile + kScanHalo) / 4];
    __shared__ uint32_t queue[4][128];
    const uint64_t t0 = (uint64_t)blockIdx.x * kScanTile;
    for (uint32_t i = threadIdx.x; i < (kScanTile + kScanHalo) / 4; i += blockDim.x) {
        const uint64_t g = t0 + 4ull * i;
        uint32_t v = 0;
        if (g + 4 <= n) {
            v = *(const uint32_t*)(in + g); // (d_in is 256-byte aligned and t0 a multiple of 4)
        } else {
            for (uint32_t k = 0; k < 4; ++k)
                if (g + k < n) v |= (uint32_t)in[g + k] << (8 * k);
        }
        tile[i] = v;
    }
    __syncthreads();
    const uint8_t* tb = (const uint8_t*)tile;
    const uint64_t tn = std::min<uint64_t>(kScanTile + kScanHalo, n - t0); // the bytes the tile holds of the piece
    const uint64_t tbytes = std::min<uint64_t>(kScanTile, n - t0);         // the bytes whose offsets it tests
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t below = (1ull << lane) - 1;
    uint32_t* q = queue[w];
    uint32_t qn = 0; // (wave-uniform)
    auto flush = [&](uint32_t m) {
        __builtin_amdgcn_wave_barrier();
        bool ok = false;
        uint32_t b = 0;
        if (lane < m) {
            b = q[lane];
            ok = inf_dynamic_ok(tb, tn, b);
        }
        const uint64_t acc = __ballot(ok);
        if (acc) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(count, (uint32_t)__popcll(acc));
            base = __shfl(base, 0);
            if (ok) {
                const uint32_t k = base + (uint32_t)__popcll(acc & below);
                if (k < cap) cand[k] = (uint32_t)(t0 * 8 + b);
            }
        }
        uint32_t rest = 0;
        if (lane + m < qn) rest = q[lane + m];
        __builtin_amdgcn_wave_barrier();
        if (lane + m < qn) q[lane] = rest;
        __builtin_amdgcn_wave_barrier();
        qn -= m;
    };
    for (uint32_t base = w * (kScanTile / 4); base < (w + 1) * (kScanTile / 4); base += 64) {
        const uint32_t j = base + lane;
        for (uint32_t k = 0; k < 8; ++k) {
            const uint32_t bit = 8 * j + k;
            InfDynHead h;
            const bool pass = j < tbytes && inf_dynamic_head(tb, tn, bit, h);
            const uint64_t m = __ballot(pass);
            if (pass) q[qn + (uint32_t)__popcll(m & below)] = bit;
            qn += (uint32_t)__popcll(m);
            if (qn >= 64) flush(64);
        }
    }
    if (qn) flush(qn);
}

// One wave per candidate segment; lane 0 decodes from bit starts[i] << shift into slot i (slot_syms symbols).
// block_min == kInfNoBlockStop: the flush mode (stop_at_flush); else block mode.
__global__ void __launch_bounds__(64) inflate_decode_kernel(const uint8_t* __restrict__ in, uint64_t n, const uint32_t* __restrict__ starts,
                                                            uint32_t shift, uint16_t* slots, uint32_t slot_syms, uint64_t block_min,
                                                            InflateSegRes* res)
{
    __shared__ InflateTables t;
    if (threadIdx.x != 0) return;
    const uint32_t i = blockIdx.x;
    uint16_t* out = slots + (uint64_t)i * slot_syms;
    const InflateRun r = inflate_run<uint16_t>(in, n, (uint64_t)starts[i] << shift, out, 0, slot_syms, true, block_min == kInfNoBlockStop, t,
                                               block_min);
    InflateSegRes q;
    q.end_bit = r.end_bit;
    q.out_len = (uint32_t)r.out_len;
    q.hole_end = r.hole_end;
    q.status = r.status;
    q.cut = (uint32_t)r.cut;
    res[i] = q;
}

__global__ void __launch_bounds__(256) inflate_fill_kernel(uint16_t* slots, uint32_t slot_syms, const InflateLink* __restrict__ links,
                                                           uint32_t first, const uint8_t* __restrict__ win, uint32_t wlen, uint32_t* flags)
{
    const uint32_t j = first + blockIdx.x;
    const InflateLink L = links[j];
    uint16_t* seg = slots + (uint64_t)L.slot * slot_syms;
    uint32_t left = 0, bad = 0;
    for (uint32_t p = threadIdx.x; p < L.hole_end; p += blockDim.x) {
        const uint32_t v = seg[p];
        if (v < kInfHole) continue;
        const int64_t g = (int64_t)L.off - (int64_t)(v - kInfHole); // the byte's offset in the piece's output
        if (g < 0) {
            if (-g > (int64_t)wlen) { ++bad; continue; }
            seg[p] = win[wlen + g];
            continue;
        }
        uint32_t k = j; // the segment that holds g: the one before, unless it is shorter than the distance
        while (k > 0 && (int64_t)links[k - 1].off > g) --k;
        if (k == 0) { ++bad; continue; } // (cannot happen: g >= 0 lies in a segment before j)
        const InflateLink& S = links[k - 1];
        const uint32_t w = slots[(uint64_t)S.slot * slot_syms + (uint64_t)(g - (int64_t)S.off)];
        if (w < kInfHole) seg[p] = (uint16_t)w;
        else ++left;
    }
    if (left) atomicAdd(&flags[0], left);
    if (bad) atomicAdd(&flags[1], bad);
}

__global__ void __launch_bounds__(256) inflate_concat_kernel(const uint16_t* __restrict__ slots, uint32_t slot_syms,
                                                             const InflateLink* __restrict__ links, uint8_t* __restrict__ out)
{
    const InflateLink L = links[blockIdx.x];
    const uint16_t* seg = slots + (uint64_t)L.slot * slot_syms;
    uint8_t* o = out + L.off;
    for (uint32_t p = threadIdx.x; p < L.len; p += blockDim.x) o[p] = (uint8_t)seg[p];
}

} // namespace

hipError_t launch_inflate_scan(const uint8_t* d_in, uint64_t n, uint32_t* d_cand, uint32_t* d_count, uint32_t cap, hipStream_t s)
{
    if (n < 4) return hipSuccess;
    const uint64_t blocks = std::min<uint64_t>((n + 255) / 256, 8192);
    inflate_scan_kernel<<<(uint32_t)blocks, 256, 0, s>>>(d_in, n, d_cand, d_count, cap);
    return hipGetLastError();
}

hipError_t launch_inflate_block_scan(const uint8_t* d_in, uint64_t n, uint32_t* d_cand, uint32_t* d_count, uint32_t cap, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (n > kInflateBlockPieceMax) return hipErrorInvalidValue;
    inflate_block_scan_kernel<<<(uint32_t)((n + kScanTile - 1) / kScanTile), 256, 0, s>>>(d_in, n, d_cand, d_count, cap);
    return hipGetLastError();
}

hipError_t launch_inflate_decode(const uint8_t* d_in, uint64_t n, const uint32_t* d_starts, uint32_t nseg, uint16_t* d_slots,
                                 InflateSegRes* d_res, hipStream_t s)
{
    if (nseg == 0) return hipSuccess;
    inflate_decode_kernel<<<nseg, 64, 0, s>>>(d_in, n, d_starts, 3, d_slots, kInflateSlotSyms, kInfNoBlockStop, d_res);
    return hipGetLastError();
}

hipError_t launch_inflate_decode_blocks(const uint8_t* d_in, uint64_t n, const uint32_t* d_bits, uint32_t nseg, uint16_t* d_slots,
                                        InflateSegRes* d_res, hipStream_t s)
{
    if (nseg == 0) return hipSuccess;
    inflate_decode_kernel<<<nseg, 64, 0, s>>>(d_in, n, d_bits, 0, d_slots, kInflateBlockSlotSyms, kInflateBlockMinOut, d_res);
    return hipGetLastError();
}

hipError_t launch_inflate_fill(uint16_t* d_slots, uint32_t slot_syms, const InflateLink* d_links, uint32_t first, uint32_t count,
                               const uint8_t* d_win, uint32_t wlen, uint32_t* d_flags, hipStream_t s)
{
    if (count == 0) return hipSuccess;
    inflate_fill_kernel<<<count, 256, 0, s>>>(d_slots, slot_syms, d_links, first, d_win, wlen, d_flags);
    return hipGetLastError();
}

hipError_t launch_inflate_concat(const uint16_t* d_slots, uint32_t slot_syms, const InflateLink* d_links, uint32_t nlinks, uint8_t* d_out,
                                 hipStream_t s)
{
    if (nlinks == 0) return hipSuccess;
    inflate_concat_kernel<<<nlinks, 256, 0, s>>>(d_slots, slot_syms, d_links, d_out);
    return hipGetLastError();
}

} // namespace snaphash
