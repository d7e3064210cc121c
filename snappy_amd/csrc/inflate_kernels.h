// inflate_kernels.h -- launchers of the GPU inflate (inflate_kernels.hip).  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace snaphash {

// What the speculative decode of one candidate segment left (inflate_core.h InflateRun, bits relative to the piece).
struct InflateSegRes {
    uint64_t end_bit;
    uint32_t out_len;
    uint32_t hole_end;
    int32_t status;
    uint32_t cut; // block mode: InflateRun::cut
};

// One segment of the linked chain: its slot, its output offset in the piece, its length and where its holes end.
struct InflateLink {
    uint64_t off;
    uint32_t slot;
    uint32_t len;
    uint32_t hole_end;
    uint32_t pad;
};

constexpr uint32_t kInflateSlotSyms = 65536 + 4096; // output symbols a slot holds (the producer's segments: 64 KiB)
// Block mode: zlib -1/-6/-9 and Go's flate end a block after 16 Ki symbols; on 16 MiB of text,
// sources and binaries one block produced 16-277 KB (tools/inflate_block_sizes.py, profiles/r06_inflate_block_sizes.jsonl),
// so a segment is one such block and a slot holds the largest with room; a block longer than that goes to the host
// decoder.  Blocks that produce fewer than kInflateBlockMinOut symbols (other encoders' short blocks) are grouped.
constexpr uint32_t kInflateBlockSlotSyms = 320u << 10;
constexpr uint64_t kInflateBlockMinOut = 16384;
constexpr uint64_t kInflateBlockPieceMax = 64ull << 20; // a piece's bit offsets fit the uint32 candidates

// Candidate segment starts in d_in[0..n): byte offsets after a possible non-final stored block (inflate_host.cpp
// flush_candidates' rule), appended unordered to d_cand; *d_count counts them all, at most cap are written.
hipError_t launch_inflate_scan(const uint8_t* d_in, uint64_t n, uint32_t* d_cand, uint32_t* d_count, uint32_t cap, hipStream_t s);
// Block mode: the bit offsets of d_in[0..n) (n <= kInflateBlockPieceMax) where inflate_core.h's inf_dynamic_ok holds -- a
// dynamic-Huffman block header inf_dynamic accepts, whole inside the piece -- appended unordered to d_cand; *d_count
// counts them all, at most cap are written.
hipError_t launch_inflate_block_scan(const uint8_t* d_in, uint64_t n, uint32_t* d_cand, uint32_t* d_count, uint32_t cap, hipStream_t s);
// One wave per segment: decodes d_in from byte d_starts[i] with holes into slot i (kInflateSlotSyms uint16 symbols).
hipError_t launch_inflate_decode(const uint8_t* d_in, uint64_t n, const uint32_t* d_starts, uint32_t nseg, uint16_t* d_slots,
                                 InflateSegRes* d_res, hipStream_t s);
// Block mode: the same from BIT d_bits[i], into slots of kInflateBlockSlotSyms, stopping at a block end past
// kInflateBlockMinOut symbols (inflate_run's block_min).
hipError_t launch_inflate_decode_blocks(const uint8_t* d_in, uint64_t n, const uint32_t* d_bits, uint32_t nseg, uint16_t* d_slots,
                                        InflateSegRes* d_res, hipStream_t s);
// Hole filling for the links first .. first+count-1 of the chain, a workgroup each: a hole takes its byte from the
// segment (or the window in front of the chain, d_win[0..wlen)) it points into, if that byte is no hole itself.
// d_flags[0] += holes left, d_flags[1] += holes that point in front of the window.  slot_syms: the slots' size.
hipError_t launch_inflate_fill(uint16_t* d_slots, uint32_t slot_syms, const InflateLink* d_links, uint32_t first, uint32_t count,
                               const uint8_t* d_win, uint32_t wlen, uint32_t* d_flags, hipStream_t s);
// The chain's symbols as bytes, laid end to end at d_out.
hipError_t launch_inflate_concat(const uint16_t* d_slots, uint32_t slot_syms, const InflateLink* d_links, uint32_t nlinks, uint8_t* d_out,
                                 hipStream_t s);

} // namespace snaphash
