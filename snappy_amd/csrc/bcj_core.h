// bcj_core.h -- the .xz format's BCJ (branch-call-jump) filters for x86 (id 0x04), PowerPC (0x05), IA64 (0x06), ARM (0x07),
// ARM-Thumb (0x08) and SPARC (0x09), shared
// by the host decoder (xz_host.cpp), the producer's host model (xz_enc_core.h), the GPU kernels (bcj_kernels.hip) and a
// host harness in tests/, the way crc_core.h serves its users.  Written from the .xz file format specification (5.3.2) and
// held byte for byte against liblzma 5.2.5's "simple" filters.
//
// A filter rewrites the relative target of a call or jump as an absolute one (encode) or back (decode), so that calls of
// one function from many places become equal bytes for LZMA2.  Positions count from the Block's first byte plus the
// filter's start_offset, modulo 2^32; nothing is carried from Block to Block.
//
// ARM and Thumb have no state: an aligned word (halfword pair) is a candidate by its own bytes, and a conversion leaves the
// bits that make it one as they are; so do PowerPC's and SPARC's words and IA64's bundles (sec. 29).  (liblzma skips the halfword behind a Thumb hit; that position could not pass the
// test: its b[1] is the hit's b[3], 0xF8 | x, where 0xF0 | x is asked for.)  So they are a lane a word, in place.
//
// x86 is a state machine (prev_mask, the position of the last 0xE8 / 0xE9 seen) whose every decision reads bytes no
// conversion has written: a conversion at j writes j+1 .. j+4 and the walk resumes at j+5.  A position p whose five bytes
// in front hold neither 0xE8 nor 0xE9 (bytes in front of the Block count as clean) is a RESTART POINT: the walk reaches it
// -- it lies inside no conversion, whose first byte would be one of the five -- and reaches it with prev_mask as good as
// zero, because the next opcode byte is more than five bytes from the last.  The kernels cut the Block at such points
// (bcj_x86_first_point, bcj_x86_walk): stretches of kBcjStretch bytes, each stretch's first restart point begins an owner's
// walk, which ends at the next owner's point; a stretch without one belongs to the owner in front.  A conversion at j needs
// j <= e - 6 for the next point e, so it writes nothing at or past e and reads nothing there: the walks run side by side in
// place, and the work is linear in the input whatever the data.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BCJ_HD __host__ __device__ inline
#else
#define BCJ_HD inline
#endif

namespace snaphash {

enum : uint32_t { kBcjNone = 0, kXzDelta = 3, kBcjX86 = 4, kBcjPowerPc = 5, kBcjIa64 = 6, kBcjArm = 7, kBcjThumb = 8, kBcjSparc = 9 }; // the format's filter ids
constexpr uint32_t kBcjStretch = 256;                                        // bytes a lane owns in the kernels
constexpr uint32_t kBcjNoPoint = 0xffffffffu;                                // a stretch without a restart point

BCJ_HD bool bcj_filter_valid(uint32_t f) { return f == kBcjX86 || f == kBcjArm || f == kBcjThumb; } // the three of sec. 25
// every filter liblzma 5.2.5 takes in front of LZMA2 (sec. 29): Delta (delta_core.h) and the six BCJ filters
BCJ_HD bool xz_filter_valid(uint32_t f) { return f >= kXzDelta && f <= kBcjSparc; }
// a start_offset must be a multiple of this (liblzma answers LZMA_OPTIONS_ERROR otherwise)
BCJ_HD uint32_t bcj_alignment(uint32_t f)
{
    return f == kBcjIa64 ? 16 : (f == kBcjArm || f == kBcjPowerPc || f == kBcjSparc) ? 4 : f == kBcjThumb ? 2 : 1;
}

// ---- ARM: the aligned word at b[i .. i+4), i % 4 == 0, i + 4 <= len; pos = start_offset + i ---------------------------------
BCJ_HD void bcj_arm_at(uint8_t* b, uint64_t i, uint32_t pos, bool encode)
{
    if (b[i + 3] != 0xEB) return;
    uint32_t src = ((uint32_t)b[i + 2] << 16) | ((uint32_t)b[i + 1] << 8) | b[i];
    src <<= 2;
    uint32_t dest = encode ? pos + 8 + src : src - (pos + 8);
    dest >>= 2;
    b[i + 2] = (uint8_t)(dest >> 16);
    b[i + 1] = (uint8_t)(dest >> 8);
    b[i] = (uint8_t)dest;
}

// ---- Thumb: the halfword pair at b[i .. i+4), i % 2 == 0, i + 4 <= len -------------------------------------------------------
BCJ_HD void bcj_thumb_at(uint8_t* b, uint64_t i, uint32_t pos, bool encode)
{
    if ((b[i + 1] & 0xF8) != 0xF0 || (b[i + 3] & 0xF8) != 0xF8) return;
    uint32_t src = (((uint32_t)b[i + 1] & 7) << 19) | ((uint32_t)b[i] << 11) | (((uint32_t)b[i + 3] & 7) << 8) | b[i + 2];
    src <<= 1;
    uint32_t dest = encode ? pos + 4 + src : src - (pos + 4);
    dest >>= 1;
    b[i + 1] = (uint8_t)(0xF0 | ((dest >> 19) & 7));
    b[i] = (uint8_t)(dest >> 11);
    b[i + 3] = (uint8_t)(0xF8 | ((dest >> 8) & 7));
    b[i + 2] = (uint8_t)dest;
}

// ---- PowerPC: the aligned big-endian word at b[i .. i+4), i % 4 == 0, i + 4 <= len; pos = start_offset + i (B/BL with AA = 0,
// LK = 1: the 24-bit word offset under the opcode's six bits) -------------------------------------------------------------------
BCJ_HD void bcj_powerpc_at(uint8_t* b, uint64_t i, uint32_t pos, bool encode)
{
    if ((b[i] >> 2) != 0x12 || (b[i + 3] & 3) != 1) return;
    const uint32_t src = (((uint32_t)b[i] & 3) << 24) | ((uint32_t)b[i + 1] << 16) | ((uint32_t)b[i + 2] << 8) | (b[i + 3] & 0xFCu);
    const uint32_t dest = encode ? pos + src : src - pos;
    b[i] = (uint8_t)(0x48 | ((dest >> 24) & 3));
    b[i + 1] = (uint8_t)(dest >> 16);
    b[i + 2] = (uint8_t)(dest >> 8);
    b[i + 3] = (uint8_t)((b[i + 3] & 3) | (dest & 0xFC));
}

// ---- SPARC: the aligned big-endian word (CALL, whose 30-bit displacement is a sign extension of 22 bits in both forms) -------
BCJ_HD void bcj_sparc_at(uint8_t* b, uint64_t i, uint32_t pos, bool encode)
{
    if (!((b[i] == 0x40 && (b[i + 1] & 0xC0) == 0) || (b[i] == 0x7F && (b[i + 1] & 0xC0) == 0xC0))) return;
    uint32_t src = ((uint32_t)b[i] << 24) | ((uint32_t)b[i + 1] << 16) | ((uint32_t)b[i + 2] << 8) | b[i + 3];
    src <<= 2;
    uint32_t dest = encode ? pos + src : src - pos;
    dest >>= 2;
    dest = (((0u - ((dest >> 22) & 1)) << 22) & 0x3FFFFFFFu) | (dest & 0x3FFFFFu) | 0x40000000u;
    b[i] = (uint8_t)(dest >> 24);
    b[i + 1] = (uint8_t)(dest >> 16);
    b[i + 2] = (uint8_t)(dest >> 8);
    b[i + 3] = (uint8_t)dest;
}

// ---- IA64: the 16-byte bundle at b[i .. i+16), i % 16 == 0, i + 16 <= len: a template of 5 bits and three slots of 41; the
// template says which slots may hold a branch (bit s of the mask).  The slots share bytes (5 and 10): one lane takes the
// bundle and its slots in order, each reading what the one in front wrote -----------------------------------------------------
BCJ_HD uint32_t bcj_ia64_mask(uint32_t templ)
{
    // templates 0x10 .. 0x1F, a nibble each: 4,4,6,6,0,0,7,7,4,4,0,0,4,4,0,0 (the sixteen in front have none)
    return templ < 16 ? 0 : (uint32_t)((0x0044004477006644ull >> (4 * (templ - 16))) & 0xF);
}
BCJ_HD void bcj_ia64_at(uint8_t* b, uint64_t i, uint32_t pos, bool encode)
{
    const uint32_t mask = bcj_ia64_mask(b[i] & 0x1F);
    for (uint32_t slot = 0, bit = 5; slot < 3; ++slot, bit += 41) {
        if (!((mask >> slot) & 1)) continue;
        uint8_t* q = b + i + (bit >> 3);
        const uint32_t res = bit & 7;
        uint64_t ins = 0;
        for (uint32_t j = 0; j < 6; ++j) ins |= (uint64_t)q[j] << (8 * j);
        uint64_t n = ins >> res;
        if (((n >> 37) & 0xF) != 5 || ((n >> 9) & 7) != 0) continue;
        uint32_t src = (uint32_t)((n >> 13) & 0xFFFFF) | ((uint32_t)((n >> 36) & 1) << 20);
        src <<= 4;
        uint32_t dest = encode ? pos + src : src - pos;
        dest >>= 4;
        n &= ~(0x8FFFFFull << 13);
        n |= (uint64_t)(dest & 0xFFFFF) << 13;
        n |= (uint64_t)(dest & 0x100000) << (36 - 20);
        ins = (ins & ((1ull << res) - 1)) | (n << res);
        for (uint32_t j = 0; j < 6; ++j) q[j] = (uint8_t)(ins >> (8 * j));
    }
}

// ---- x86 ---------------------------------------------------------------------------------------------------------------------
BCJ_HD bool bcj_x86_op(uint32_t b) { return (b & 0xFE) == 0xE8; }       // CALL rel32, JMP rel32
BCJ_HD bool bcj_x86_ms(uint32_t b) { return b == 0 || b == 0xFF; }      // a high byte that keeps a target near

// The first restart point in [s, e) of the Block b[0 .. len), e <= len; kBcjNoPoint-like ~0 when there is none.  Reads
// b[max(s, 5) - 5 .. e - 1) at most.
BCJ_HD uint64_t bcj_x86_first_point(const uint8_t* b, uint64_t s, uint64_t e)
{
    const uint64_t lo = s >= 5 ? s - 5 : 0;
    uint32_t clean = s >= 5 ? 0 : (uint32_t)(5 - s); // the bytes in front of the Block
    for (uint64_t q = lo; q < s; ++q) clean = bcj_x86_op(b[q]) ? 0 : clean + 1;
    for (uint64_t p = s; p < e; ++p) {
        if (clean >= 5) return p;
        clean = bcj_x86_op(b[p]) ? 0 : clean + 1;
    }
    return ~0ull;
}

// liblzma's x86_code over the positions [s, e) of the Block b[0 .. len), begun at the restart point s (0 is one) with a
// fresh state; e: the next restart point taken, or len.  The Block's last four bytes are never a conversion's first.
BCJ_HD void bcj_x86_walk(uint8_t* b, uint64_t len, uint64_t s, uint64_t e, uint32_t start_offset, bool encode)
{
    if (len < 5) return;
    const uint64_t limit = len - 5;
    if (e > limit + 1) e = limit + 1;
    uint32_t prev_mask = 0;
    uint64_t prev_pos = s - 5; // (may wrap: only differences are taken)
    uint64_t pos = s;
    while (pos < e) {
        if (!bcj_x86_op(b[pos])) {
            ++pos;
            continue;
        }
        const uint64_t offset = pos - prev_pos;
        prev_pos = pos;
        if (offset > 5) {
            prev_mask = 0;
        } else {
            for (uint32_t i = 0; i < (uint32_t)offset; ++i) prev_mask = (prev_mask & 0x77) << 1;
        }
        uint32_t top = b[pos + 4];
        // the masks 0, 1, 2 and 4 (of prev_mask >> 1) allow a conversion
        if (bcj_x86_ms(top) && ((0x17u >> ((prev_mask >> 1) & 7)) & 1) && (prev_mask >> 1) < 0x10) {
            uint32_t src = (top << 24) | ((uint32_t)b[pos + 3] << 16) | ((uint32_t)b[pos + 2] << 8) | b[pos + 1];
            const uint32_t here = start_offset + (uint32_t)pos + 5;
            uint32_t dest;
            for (;;) {
                dest = encode ? src + here : src - here;
                if (prev_mask == 0) break;
                const uint32_t i = (0x33332210u >> (4 * ((prev_mask >> 1) & 7))) & 0xF; // 0 1 2 2 3 3 3 3
                top = (uint8_t)(dest >> (24 - i * 8));
                if (!bcj_x86_ms(top)) break;
                src = dest ^ ((1u << (32 - i * 8)) - 1);
            }
            b[pos + 4] = (uint8_t)(~(((dest >> 24) & 1) - 1));
            b[pos + 3] = (uint8_t)(dest >> 16);
            b[pos + 2] = (uint8_t)(dest >> 8);
            b[pos + 1] = (uint8_t)dest;
            pos += 5;
            prev_mask = 0;
        } else {
            ++pos;
            prev_mask |= 1;
            if (bcj_x86_ms(top)) prev_mask |= 0x10;
        }
    }
}

// ---- a whole Block on one thread, in place ----------------------------------------------------------------------------------
// filter: one of the six BCJ ids (anything else, Delta included: nothing is done).  The Block's last 4 bytes (x86), incomplete
// word (ARM, PowerPC, SPARC), halfword pair (Thumb) or bundle (IA64) stay as they are.
BCJ_HD void bcj_block(uint32_t filter, bool encode, uint8_t* b, uint64_t len, uint32_t start_offset)
{
    if (filter == kBcjX86) {
        bcj_x86_walk(b, len, 0, len, start_offset, encode);
    } else if (filter == kBcjArm) {
        for (uint64_t i = 0; i + 4 <= len; i += 4) bcj_arm_at(b, i, start_offset + (uint32_t)i, encode);
    } else if (filter == kBcjThumb) {
        for (uint64_t i = 0; i + 4 <= len; i += 2) bcj_thumb_at(b, i, start_offset + (uint32_t)i, encode);
    } else if (filter == kBcjPowerPc) {
        for (uint64_t i = 0; i + 4 <= len; i += 4) bcj_powerpc_at(b, i, start_offset + (uint32_t)i, encode);
    } else if (filter == kBcjSparc) {
        for (uint64_t i = 0; i + 4 <= len; i += 4) bcj_sparc_at(b, i, start_offset + (uint32_t)i, encode);
    } else if (filter == kBcjIa64) {
        for (uint64_t i = 0; i + 16 <= len; i += 16) bcj_ia64_at(b, i, start_offset + (uint32_t)i, encode);
    }
}

// ---- the kernels' cut, a stretch at a time (bcj_kernels.hip runs these two a lane a stretch; the host harness runs them in
// a loop and must see bcj_block's bytes) ---------------------------------------------------------------------------------------

// pass 1: stretch k's first restart point, relative to the stretch, or kBcjNoPoint
BCJ_HD uint32_t bcj_x86_stretch_point(const uint8_t* b, uint64_t len, uint64_t k, uint32_t stretch)
{
    const uint64_t s = k * stretch, e = s + stretch < len ? s + stretch : len;
    const uint64_t p = bcj_x86_first_point(b, s, e);
    return p == ~0ull ? kBcjNoPoint : (uint32_t)(p - s);
}
// pass 2: stretch k's share of the Block of nk stretches, points[0 .. nk) from pass 1
BCJ_HD void bcj_stretch_apply(uint32_t filter, bool encode, uint8_t* b, uint64_t len, uint64_t k, uint64_t nk, uint32_t stretch,
                              const uint32_t* points, uint32_t start_offset)
{
    const uint64_t s = k * stretch, e = s + stretch < len ? s + stretch : len;
    if (filter == kBcjX86) {
        if (points[k] == kBcjNoPoint) return; // the owner in front walks through
        uint64_t end = len;
        for (uint64_t v = k + 1; v < nk; ++v)
            if (points[v] != kBcjNoPoint) {
                end = v * stretch + points[v];
                break;
            }
        bcj_x86_walk(b, len, s + points[k], end, start_offset, encode);
    } else if (filter == kBcjArm) {
        for (uint64_t i = s; i < e && i + 4 <= len; i += 4) bcj_arm_at(b, i, start_offset + (uint32_t)i, encode);
    } else if (filter == kBcjThumb) {
        for (uint64_t i = s; i < e && i + 4 <= len; i += 2) bcj_thumb_at(b, i, start_offset + (uint32_t)i, encode);
    } else if (filter == kBcjPowerPc) { // (a stretch is a multiple of 16 bytes from the range's first: no word or bundle straddles one)
        for (uint64_t i = s; i < e && i + 4 <= len; i += 4) bcj_powerpc_at(b, i, start_offset + (uint32_t)i, encode);
    } else if (filter == kBcjSparc) {
        for (uint64_t i = s; i < e && i + 4 <= len; i += 4) bcj_sparc_at(b, i, start_offset + (uint32_t)i, encode);
    } else if (filter == kBcjIa64) {
        for (uint64_t i = s; i < e && i + 16 <= len; i += 16) bcj_ia64_at(b, i, start_offset + (uint32_t)i, encode);
    }
}

} // namespace snaphash
