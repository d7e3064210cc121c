// xz_core.h -- the .xz container and the LZMA2 / LZMA decoder, shared by the host decoder (xz_host.cpp), the GPU kernel
// (xz_kernels.hip) and a host harness in tests/, the way bzip2_core.h and inflate_core.h serve their decoders.  Written
// from the .xz file format specification (version 1.0.4) and the LZMA algorithm description; the container parsing is
// host-only, the decoder is host + device (XZ_HD).
//
// A .xz file is a sequence of Streams (with Stream Padding of four zero bytes at a time between and after them); a Stream
// is a header, Blocks, an Index and a footer.  A Block's LZMA2 data needs no byte of any other Block, and the Index lists
// every Block's unpadded and uncompressed size: xz_plan walks the Streams from the END of the buffer (footer, backward
// size, Index), which gives every Block's input offset and its offset in the whole result before a byte is decoded, then
// checks every Block header against its Index record.  The Blocks are then decoded side by side, each straight to its
// final place -- which is also its dictionary.
//
// The verdict is liblzma's (as Python's lzma module drives it): what it accepts this accepts with the same bytes, what it
// refuses this refuses.  Where the texts leave a doubt it was settled against liblzma 5.2.5:
//   - a match that would run past its chunk's uncompressed size is refused (liblzma: LZMA_DATA_ERROR; it does not carry the
//     rest of the copy into the next chunk);
//   - the first of a chunk's five range coder start bytes must be zero (liblzma refuses a chunk where it is not);
//   - when a chunk's output is complete the range decoder is normalised once more; the chunk's compressed size must then
//     be consumed exactly and the value left in `code` must be zero (liblzma's rc_is_finished);
//   - an end-of-payload marker (distance 0xFFFFFFFF) is refused in LZMA2;
//   - a distance is valid while it is at most the bytes produced since the last dictionary reset and at most the
//     dictionary size of the Block header; a short rep or rep match before any byte is refused by the same rule;
//   - Block header sizes that are present must equal what the decoder finds, and the Index record must equal both.
// Python's lzma.decompress wrapper (not liblzma) drops trailing bytes that do not begin a Stream and does not read Stream
// Padding at all; here, as in liblzma's LZMA_CONCATENATED mode and the xz tool, padding is read and junk is refused.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define XZ_HD __host__ __device__ inline
#else
#define XZ_HD inline
#endif

#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "bcj_core.h"
#include "delta_core.h"

namespace snaphash {

// ---- LZMA ------------------------------------------------------------------------------------------------------------

constexpr uint32_t kLzmaLitBase = 1846;                        // the probabilities in front of the literal coder
constexpr uint32_t kLzmaProbsMax = kLzmaLitBase + (0x300 << 4); // lc + lp <= 4: 14 134 entries of 16 bits
constexpr uint32_t kLzmaProbInit = 1024;
constexpr uint32_t kLzma2ChunkMax = 1u << 21; // a chunk's uncompressed size, at most
constexpr uint32_t kLzmaMatchMax = 273;
constexpr uint32_t kXzWave = 64;              // the lanes that copy a match body in the kernel

enum : uint32_t { // offsets into the probability array
    kPIsMatch = 0, kPIsRep = 192, kPIsRepG0 = 204, kPIsRepG1 = 216, kPIsRepG2 = 228, kPIsRep0Long = 240, kPPosSlot = 432,
    kPSpecPos = 688, kPAlign = 802, kPLen = 818, kPRepLen = 1332
};
enum : uint32_t { kLenChoice = 0, kLenChoice2 = 1, kLenLow = 2, kLenMid = 130, kLenHigh = 258 };

enum : int { kXzOk = 0, kXzBad = 1 }; // a Block's status

XZ_HD uint32_t lzma_probs_count(uint32_t lc, uint32_t lp) { return kLzmaLitBase + (0x300u << (lc + lp)); }

// where byte i of a match body of distance dist at pos comes from: the source repeats when dist < len, which is legal
// because [pos - dist, pos) is written before any byte of the body
XZ_HD uint64_t xz_copy_src(uint64_t pos, uint32_t dist, uint32_t i) { return pos - dist + (i < dist ? i : i % dist); }
// lane `lane`'s share of the body, a byte every kXzWave; returns the last byte it wrote (the wave's last byte is lane
// (len - 1) % kXzWave's)
XZ_HD uint32_t xz_copy_lane(uint8_t* out, uint64_t pos, uint32_t dist, uint32_t len, uint32_t lane)
{
    uint32_t last = 0;
    for (uint32_t i = lane; i < len; i += kXzWave) {
        last = out[xz_copy_src(pos, dist, i)];
        out[pos + i] = (uint8_t)last;
    }
    return last;
}

// The decoder's registers.  dpos counts the bytes since the last dictionary reset (the position the literal and position
// states are taken from, and the bound of a distance).
struct LzmaDec {
    uint32_t range, code;
    uint32_t state;
    uint32_t rep0, rep1, rep2, rep3; // distances - 1
    uint32_t lc, lp_mask, pb_mask;
    uint32_t prev;                   // the byte before pos
    uint32_t dict_size;
};

// What a run ends with.
enum : int { kRunChunkEnd = 0, kRunMatch = 1, kRunError = 2 };

// IO gives the decoder its bytes: uint32_t next() (the chunk's next compressed byte; past the chunk's end it returns 0 and
// remembers it, bool over()), uint32_t out_at(uint64_t) (a byte of the Block's output already written) and
// void put(uint64_t, uint32_t).
template <class IO> XZ_HD uint32_t rc_bit(LzmaDec& d, IO& io, uint16_t* p)
{
    const uint32_t v = *p;
    const uint32_t bound = (d.range >> 11) * v;
    uint32_t bit;
    if (d.code < bound) {
        d.range = bound;
        *p = (uint16_t)(v + ((2048 - v) >> 5));
        bit = 0;
    } else {
        d.range -= bound;
        d.code -= bound;
        *p = (uint16_t)(v - (v >> 5));
        bit = 1;
    }
    if (d.range < (1u << 24)) {
        d.range <<= 8;
        d.code = (d.code << 8) | io.next();
    }
    return bit;
}
template <class IO> XZ_HD uint32_t rc_tree(LzmaDec& d, IO& io, uint16_t* p, uint32_t bits)
{
    uint32_t m = 1;
    for (uint32_t i = 0; i < bits; ++i) m = (m << 1) | rc_bit(d, io, p + m);
    return m - (1u << bits);
}
template <class IO> XZ_HD uint32_t rc_tree_rev(LzmaDec& d, IO& io, uint16_t* p, uint32_t bits)
{
    uint32_t m = 1, r = 0;
    for (uint32_t i = 0; i < bits; ++i) {
        const uint32_t b = rc_bit(d, io, p + m);
        m = (m << 1) | b;
        r |= b << i;
    }
    return r;
}
template <class IO> XZ_HD uint32_t rc_direct(LzmaDec& d, IO& io, uint32_t bits)
{
    uint32_t r = 0;
    for (uint32_t i = 0; i < bits; ++i) {
        d.range >>= 1;
        d.code -= d.range;
        const uint32_t t = 0u - (d.code >> 31);
        d.code += d.range & t;
        r = (r << 1) + (t + 1);
        if (d.range < (1u << 24)) {
            d.range <<= 8;
            d.code = (d.code << 8) | io.next();
        }
    }
    return r;
}
template <class IO> XZ_HD uint32_t lzma_len(LzmaDec& d, IO& io, uint16_t* p, uint32_t pos_state)
{
    if (!rc_bit(d, io, p + kLenChoice)) return 2 + rc_tree(d, io, p + kLenLow + (pos_state << 3), 3);
    if (!rc_bit(d, io, p + kLenChoice2)) return 10 + rc_tree(d, io, p + kLenMid + (pos_state << 3), 3);
    return 18 + rc_tree(d, io, p + kLenHigh, 8);
}

XZ_HD void lzma_reset_state(LzmaDec& d)
{
    d.state = 0;
    d.rep0 = d.rep1 = d.rep2 = d.rep3 = 0;
}
// the chunk's five start bytes; false when the first is not zero
template <class IO> XZ_HD bool lzma_rc_start(LzmaDec& d, IO& io)
{
    d.range = 0xffffffffu;
    d.code = 0;
    const uint32_t first = io.next();
    for (int i = 0; i < 4; ++i) d.code = (d.code << 8) | io.next();
    return first == 0;
}

// What a run tells about the operations it decoded (the host harness counts them; the kernel and the library pass NoOps).
struct NoOps {
    XZ_HD void lit(bool) {}
    XZ_HD void match() {}
    XZ_HD void rep(int) {}
    XZ_HD void short_rep() {}
    XZ_HD void copy(uint32_t, uint32_t, uint64_t, uint32_t) {} // distance, length, bytes since the dictionary reset, dictionary size
};

// Decodes from pos (dpos bytes after the dictionary reset) until the chunk's output is complete (kRunChunkEnd), a match
// body is due (kRunMatch: *m_dist, *m_len; the caller copies it, sets d.prev and advances) or the input is malformed
// (kRunError).  Literals and short reps are written here.  Nothing is written at or past chunk_end; the match is checked
// against chunk_end, the dictionary size and dpos before it is returned.
template <class IO, class OPS>
XZ_HD int lzma_run(LzmaDec& d, uint16_t* probs, IO& io, uint64_t& pos, uint64_t& dpos, uint64_t chunk_end, uint32_t* m_dist,
                   uint32_t* m_len, OPS& ops)
{
    while (pos < chunk_end) {
        if (io.over()) return kRunError;
        const uint32_t pos_state = (uint32_t)dpos & d.pb_mask;
        if (!rc_bit(d, io, probs + kPIsMatch + (d.state << 4) + pos_state)) {
            uint16_t* p = probs + kLzmaLitBase + 0x300u * ((((uint32_t)dpos & d.lp_mask) << d.lc) + (d.prev >> (8 - d.lc)));
            uint32_t sym = 1;
            if (d.state < 7) {
                do sym = (sym << 1) | rc_bit(d, io, p + sym);
                while (sym < 0x100);
                ops.lit(false);
            } else {
                uint32_t mb = io.out_at(pos - d.rep0 - 1), offs = 0x100;
                do {
                    mb <<= 1;
                    const uint32_t mbit = mb & offs;
                    const uint32_t b = rc_bit(d, io, p + offs + mbit + sym);
                    sym = (sym << 1) | b;
                    offs &= b ? mbit : ~mbit;
                } while (sym < 0x100);
                ops.lit(true);
            }
            d.prev = sym & 0xff;
            io.put(pos, d.prev);
            ++pos;
            ++dpos;
            d.state = d.state < 4 ? 0 : d.state < 10 ? d.state - 3 : d.state - 6;
            continue;
        }
        uint32_t len;
        if (!rc_bit(d, io, probs + kPIsRep + d.state)) {
            d.rep3 = d.rep2;
            d.rep2 = d.rep1;
            d.rep1 = d.rep0;
            len = lzma_len(d, io, probs + kPLen, pos_state);
            d.state = d.state < 7 ? 7 : 10;
            const uint32_t slot = rc_tree(d, io, probs + kPPosSlot + ((len < 6 ? len - 2 : 3) << 6), 6);
            if (slot < 4) {
                d.rep0 = slot;
            } else {
                const uint32_t nb = (slot >> 1) - 1;
                d.rep0 = (2 | (slot & 1)) << nb;
                if (slot < 14) {
                    d.rep0 += rc_tree_rev(d, io, probs + kPSpecPos + d.rep0 - slot - 1, nb);
                } else {
                    d.rep0 += rc_direct(d, io, nb - 4) << 4;
                    d.rep0 += rc_tree_rev(d, io, probs + kPAlign, 4);
                    if (d.rep0 == 0xffffffffu) return kRunError; // the end marker has no place in LZMA2
                }
            }
            ops.match();
        } else {
            if (dpos == 0) return kRunError; // a rep before any byte
            if (!rc_bit(d, io, probs + kPIsRepG0 + d.state)) {
                if (!rc_bit(d, io, probs + kPIsRep0Long + (d.state << 4) + pos_state)) {
                    if (d.rep0 >= dpos || d.rep0 >= d.dict_size) return kRunError;
                    d.state = d.state < 7 ? 9 : 11;
                    d.prev = io.out_at(pos - d.rep0 - 1);
                    io.put(pos, d.prev);
                    ++pos;
                    ++dpos;
                    ops.short_rep();
                    continue;
                }
                ops.rep(0);
            } else {
                uint32_t dist;
                if (!rc_bit(d, io, probs + kPIsRepG1 + d.state)) {
                    dist = d.rep1;
                    ops.rep(1);
                } else {
                    if (!rc_bit(d, io, probs + kPIsRepG2 + d.state)) {
                        dist = d.rep2;
                        ops.rep(2);
                    } else {
                        dist = d.rep3;
                        d.rep3 = d.rep2;
                        ops.rep(3);
                    }
                    d.rep2 = d.rep1;
                }
                d.rep1 = d.rep0;
                d.rep0 = dist;
            }
            len = lzma_len(d, io, probs + kPRepLen, pos_state);
            d.state = d.state < 7 ? 8 : 11;
        }
        if (io.over() || d.rep0 >= dpos || d.rep0 >= d.dict_size || len > chunk_end - pos) return kRunError;
        *m_dist = d.rep0 + 1;
        *m_len = len;
        return kRunMatch;
    }
    return io.over() ? kRunError : kRunChunkEnd;
}

// An LZMA2 chunk header, read from in[at .. end).  kind: 0 end, 1 uncompressed, 2 LZMA.
struct Lzma2Chunk {
    uint32_t kind, usize, csize, hdr;
    bool dict_reset, state_reset, new_props;
    uint32_t lc, lp, pb;
};
// 0, or 1 when the header is malformed or cut off.  need_dict_reset: no chunk of the Block came before; need_props: no
// LZMA chunk has carried properties since the Block began or an uncompressed chunk last reset the dictionary.
template <class RD> XZ_HD int lzma2_chunk_header(RD& rd, uint64_t at, uint64_t end, bool need_dict_reset, bool need_props, Lzma2Chunk& c)
{
    if (at >= end) return 1;
    const uint32_t ctl = rd.in_at(at);
    c.dict_reset = c.state_reset = c.new_props = false;
    c.lc = c.lp = c.pb = 0;
    c.usize = c.csize = 0;
    if (ctl == 0) { c.kind = 0; c.hdr = 1; return 0; }
    if (ctl < 0x80) {
        if (ctl > 2 || end - at < 3) return 1;
        c.kind = 1;
        c.hdr = 3;
        c.dict_reset = ctl == 1;
        if (need_dict_reset && !c.dict_reset) return 1;
        c.usize = c.csize = ((rd.in_at(at + 1) << 8) | rd.in_at(at + 2)) + 1;
        return 0;
    }
    const uint32_t mode = (ctl >> 5) & 3;
    c.kind = 2;
    c.dict_reset = mode == 3;
    c.new_props = mode >= 2;
    c.state_reset = mode >= 1;
    c.hdr = c.new_props ? 6 : 5;
    if (end - at < c.hdr) return 1;
    if (need_dict_reset && !c.dict_reset) return 1;
    if (need_props && !c.new_props) return 1;
    c.usize = (((ctl & 0x1f) << 16) | (rd.in_at(at + 1) << 8) | rd.in_at(at + 2)) + 1;
    c.csize = ((rd.in_at(at + 3) << 8) | rd.in_at(at + 4)) + 1;
    if (c.new_props) {
        uint32_t pr = rd.in_at(at + 5);
        if (pr > 4 * 45 + 4 * 9 + 8) return 1;
        c.pb = pr / 45;
        pr -= c.pb * 45;
        c.lp = pr / 9;
        c.lc = pr - c.lp * 9;
        if (c.lc + c.lp > 4) return 1;
    }
    return 0;
}

// ---- the host's IO and a whole Block on one thread -------------------------------------------------------------------

struct XzHostIO {
    const uint8_t* in;
    uint64_t ip, iend; // the chunk's compressed bytes: in[ip .. iend)
    uint8_t* out;      // the Block's output (index 0 = the Block's first byte)
    bool ov;
    uint32_t next()
    {
        if (ip < iend) return in[ip++];
        ov = true;
        return 0;
    }
    bool over() const { return ov; }
    uint32_t out_at(uint64_t p) const { return out[p]; }
    void put(uint64_t p, uint32_t b) { out[p] = (uint8_t)b; }
    uint32_t in_at(uint64_t p) const { return in[p]; }
};

struct Lzma2Trace { // what the host harness wants to know about a Block's chunks
    std::vector<uint8_t> controls;
    std::vector<uint32_t> props; // lc | lp << 4 | pb << 8 of every chunk that set them
    std::vector<uint32_t> usizes;
};

// The LZMA2 data in[0 .. in_len) into out[0 .. out_len): kXzOk when it ends with the end byte exactly at in_len having
// produced exactly out_len bytes.  probs: kLzmaProbsMax entries of scratch.
template <class OPS>
inline int lzma2_block_host(const uint8_t* in, uint64_t in_len, uint8_t* out, uint64_t out_len, uint32_t dict_size, uint16_t* probs,
                            OPS& ops, Lzma2Trace* trace = nullptr)
{
    XzHostIO io{in, 0, 0, out, false};
    LzmaDec d{};
    d.dict_size = dict_size;
    uint64_t at = 0, pos = 0, dpos = 0;
    bool need_dict = true, need_props = true;
    for (;;) {
        Lzma2Chunk c;
        if (lzma2_chunk_header(io, at, in_len, need_dict, need_props, c)) return kXzBad;
        if (trace) trace->controls.push_back(in[at]);
        if (c.kind == 0) return (at + 1 == in_len && pos == out_len) ? kXzOk : kXzBad;
        at += c.hdr;
        if (c.csize > in_len - at || c.usize > out_len - pos) return kXzBad;
        if (trace) trace->usizes.push_back(c.usize);
        if (c.dict_reset) { dpos = 0; need_props = true; }
        need_dict = false;
        if (c.kind == 1) {
            memcpy(out + pos, in + at, c.usize);
            pos += c.usize;
            dpos += c.usize;
            at += c.csize;
            d.prev = out[pos - 1];
            continue; // (liblzma leaves the LZMA state as it is: only a later chunk's control byte resets it)
        }
        if (c.new_props) {
            d.lc = c.lc;
            d.lp_mask = (1u << c.lp) - 1;
            d.pb_mask = (1u << c.pb) - 1;
            need_props = false;
            if (trace) trace->props.push_back(c.lc | c.lp << 4 | c.pb << 8);
        }
        if (c.state_reset) {
            lzma_reset_state(d);
            const uint32_t np = lzma_probs_count(d.lc, (uint32_t)__builtin_popcount(d.lp_mask));
            for (uint32_t i = 0; i < np; ++i) probs[i] = kLzmaProbInit;
        }
        if (dpos == 0) d.prev = 0;
        io.ip = at;
        io.iend = at + c.csize;
        io.ov = false;
        if (!lzma_rc_start(d, io)) return kXzBad;
        const uint64_t chunk_end = pos + c.usize;
        for (;;) {
            uint32_t dist = 0, len = 0;
            const int r = lzma_run(d, probs, io, pos, dpos, chunk_end, &dist, &len, ops);
            if (r == kRunError) return kXzBad;
            if (r == kRunChunkEnd) break;
            ops.copy(dist, len, dpos, d.dict_size);
            for (uint32_t i = 0; i < len; ++i) out[pos + i] = out[pos + i - dist];
            pos += len;
            dpos += len;
            d.prev = out[pos - 1];
        }
        if (io.ov || io.ip != io.iend || d.code != 0) return kXzBad;
        at += c.csize;
    }
}

// ---- the container -----------------------------------------------------------------------------------------------------

enum : int { kXzPlanOk = 0, kXzPlanFormat = 1, kXzPlanUnsupported = 2 };
enum : uint32_t { kXzCheckNone = 0, kXzCheckCrc32 = 1, kXzCheckCrc64 = 4, kXzCheckSha256 = 10 };

struct XzBlock {
    uint64_t in_off = 0;   // the LZMA2 data, in the file
    uint64_t in_len = 0;
    uint64_t out_off = 0;  // in the whole result
    uint64_t out_len = 0;
    uint64_t check_off = 0; // the Check field, in the file
    uint32_t check = 0;     // its id
    uint32_t dict_size = 0;
    uint32_t bcj = 0;       // the BCJ filter in front of LZMA2 (kBcjX86 / kBcjArm / kBcjThumb), 0: none; only xz_plan(allow_bcj)
    uint32_t bcj_start = 0; // sets it, with the filter's start_offset
    // the chain in front of LZMA2 as the header names it, first filter first (xz_plan with kXzChainBcj: at most the one above;
    // with kXzChainAny: up to three of Delta and the six BCJ filters).  fparam: a BCJ filter's start_offset, Delta's distance
    uint32_t nfilt = 0;
    uint32_t filt[3] = {0, 0, 0};
    uint32_t fparam[3] = {0, 0, 0};
};

// which filter chains xz_block_header and xz_plan take beside one LZMA2 (a bool converts: false / true are the first two)
enum : int { kXzChainNone = 0, kXzChainBcj = 1, kXzChainAny = 2 };

// A Block's chain undone on one thread, in place: the filter nearest LZMA2 first
inline void xz_chain_undo(const XzBlock& b, uint8_t* out)
{
    for (uint32_t k = b.nfilt; k-- > 0;) {
        if (b.filt[k] == kXzDelta) delta_block(false, out, b.out_len, b.fparam[k]);
        else bcj_block(b.filt[k], false, out, b.out_len, b.fparam[k]);
    }
}

inline uint32_t xz_check_size(uint32_t id) { return id == 0 ? 0 : id <= 3 ? 4 : id <= 6 ? 8 : id <= 9 ? 16 : id <= 12 ? 32 : 64; }

// CRC-32 (gzip's) of the container's small fields
inline uint32_t xz_crc32(const uint8_t* p, uint64_t n)
{
    static const struct T {
        uint32_t t[256];
        T()
        {
            for (uint32_t b = 0; b < 256; ++b) {
                uint32_t c = b;
                for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1) ? 0xEDB88320u : 0);
                t[b] = c;
            }
        }
    } tab;
    uint32_t c = 0xffffffffu;
    for (uint64_t i = 0; i < n; ++i) c = (c >> 8) ^ tab.t[(c ^ p[i]) & 0xff];
    return ~c;
}
inline uint32_t xz_le32(const uint8_t* p) { return p[0] | p[1] << 8 | p[2] << 16 | (uint32_t)p[3] << 24; }

// a variable-length integer of p[*at .. end): 1 to 9 bytes, at most 63 bits, no padding zero byte at its end
inline bool xz_vli(const uint8_t* p, uint64_t* at, uint64_t end, uint64_t* v)
{
    *v = 0;
    for (uint32_t i = 0; i < 9; ++i) {
        if (*at >= end) return false;
        const uint8_t b = p[(*at)++];
        *v |= (uint64_t)(b & 0x7f) << (7 * i);
        if (!(b & 0x80)) return !(b == 0 && i > 0);
    }
    return false;
}

// an LZMA2 dictionary size byte (<= 40)
inline uint32_t xz_dict_size(uint32_t b) { return b == 40 ? 0xffffffffu : (2u | (b & 1)) << (b / 2 + 11); }

// A Block header at p[at ..): its size, the sizes it states (or ~0), the dictionary size.  kXzPlanUnsupported with *why
// for a filter chain other than one LZMA2 -- or, with allow_bcj, other than one LZMA2 or one BCJ filter (x86, ARM, Thumb)
// in front of one LZMA2: *bcj / *bcj_start then say which (0: none).  Such a filter's properties are 0 bytes or 4 (its
// start_offset, a multiple of the filter's alignment); liblzma refuses anything else, and so does this: kXzPlanFormat.
// With chains == kXzChainAny (and chain != nullptr) every chain liblzma 5.2.5 reads: up to three of Delta (0x03, one byte of
// properties: the distance less one) and the BCJ filters 0x04 .. 0x09 in any order in front of one LZMA2; *chain's nfilt,
// filt and fparam then hold it (with kXzChainBcj too), and *bcj / *bcj_start a chain of one of x86, ARM, Thumb as before.
inline int xz_block_header(const uint8_t* p, uint64_t at, uint64_t end, uint64_t* hdr, uint64_t* csize, uint64_t* usize, uint32_t* dict,
                           std::string& why, int chains = kXzChainNone, uint32_t* bcj = nullptr, uint32_t* bcj_start = nullptr,
                           XzBlock* chain = nullptr)
{
    if (at >= end || p[at] == 0) return kXzPlanFormat;
    const uint64_t hs = ((uint64_t)p[at] + 1) * 4;
    if (hs > end - at) return kXzPlanFormat;
    if (xz_crc32(p + at, hs - 4) != xz_le32(p + at + hs - 4)) return kXzPlanFormat;
    const uint8_t flags = p[at + 1];
    if (flags & 0x3c) return kXzPlanFormat; // reserved bits
    const uint32_t nf = (flags & 3) + 1;
    uint64_t q = at + 2;
    const uint64_t he = at + hs - 4;
    *csize = *usize = ~0ull;
    if (flags & 0x40) {
        if (!xz_vli(p, &q, he, csize) || *csize == 0) return kXzPlanFormat;
    }
    if (flags & 0x80) {
        if (!xz_vli(p, &q, he, usize)) return kXzPlanFormat;
    }
    bool unsupported = false;
    uint64_t bad_id = 0; // the first filter of the chain that is not LZMA2
    uint32_t dict_byte = 0;
    uint32_t others = 0; // the filters that are not LZMA2
    uint64_t first_id = 0, first_ps = 0, first_at = 0;
    uint64_t ids[4] = {0, 0, 0, 0}, pss[4] = {0, 0, 0, 0}, ats[4] = {0, 0, 0, 0};
    for (uint32_t f = 0; f < nf; ++f) {
        uint64_t id, ps;
        if (!xz_vli(p, &q, he, &id) || !xz_vli(p, &q, he, &ps) || ps > he - q) return kXzPlanFormat;
        if (id >= (1ull << 62)) return kXzPlanFormat;
        if (id != 0x21 && !unsupported) { unsupported = true; bad_id = id; }
        others += id != 0x21;
        if (f == 0) { first_id = id; first_ps = ps; first_at = q; }
        ids[f] = id; pss[f] = ps; ats[f] = q;
        if (id == 0x21) {
            if (f + 1 != nf || ps != 1) return kXzPlanFormat; // LZMA2 is the last filter and has one byte of properties
            dict_byte = p[q];
            if (dict_byte > 40) return kXzPlanFormat;
        }
        q += ps;
    }
    for (; q < he; ++q)
        if (p[q]) return kXzPlanFormat;
    if (bcj) *bcj = *bcj_start = 0;
    if (chain) chain->nfilt = 0;
    if (unsupported && chains == kXzChainAny && bcj && chain && others == nf - 1) { // (LZMA2 is there, and the loop held it to the last place)
        bool known = true;
        for (uint32_t f = 0; f + 1 < nf && known; ++f)
            if (!xz_filter_valid((uint32_t)(ids[f] < 64 ? ids[f] : 0))) { known = false; bad_id = ids[f]; } // (the first one this library lacks is named)
        if (known) {
            for (uint32_t f = 0; f + 1 < nf; ++f) {
                uint32_t param;
                if (ids[f] == kXzDelta) {
                    if (pss[f] != 1) return kXzPlanFormat;
                    param = (uint32_t)p[ats[f]] + 1;
                } else {
                    if (pss[f] != 0 && pss[f] != 4) return kXzPlanFormat;
                    param = pss[f] ? xz_le32(p + ats[f]) : 0;
                    if (param & (bcj_alignment((uint32_t)ids[f]) - 1)) return kXzPlanFormat;
                }
                chain->filt[f] = (uint32_t)ids[f];
                chain->fparam[f] = param;
            }
            chain->nfilt = nf - 1;
            if (nf == 2 && bcj_filter_valid(chain->filt[0])) { *bcj = chain->filt[0]; *bcj_start = chain->fparam[0]; }
            unsupported = false;
        }
    }
    if (unsupported && chains == kXzChainBcj && bcj && nf == 2 && others == 1 && bcj_filter_valid((uint32_t)first_id)) {
        // (the second is LZMA2: it is not among `others`)
        if (first_ps != 0 && first_ps != 4) return kXzPlanFormat;
        const uint32_t start = first_ps ? xz_le32(p + first_at) : 0;
        if (start & (bcj_alignment((uint32_t)first_id) - 1)) return kXzPlanFormat;
        *bcj = (uint32_t)first_id;
        *bcj_start = start;
        if (chain) { chain->nfilt = 1; chain->filt[0] = *bcj; chain->fparam[0] = start; }
        unsupported = false;
    }
    if (unsupported) { // (the first one is named: one is enough to hand the file back)
        char b[64];
        snprintf(b, sizeof b, "xz: unsupported filter 0x%02llX", (unsigned long long)bad_id);
        why = b;
        return kXzPlanUnsupported;
    }
    *hdr = hs;
    *dict = xz_dict_size(dict_byte);
    return kXzPlanOk;
}

// Every Block of every Stream of p[0 .. n), in order, and the length of the whole result.  chains: as in xz_block_header.
inline int xz_plan(const uint8_t* p, uint64_t n, std::vector<XzBlock>& blocks, uint64_t* total, std::string& why, int chains = kXzChainNone)
{
    blocks.clear();
    *total = 0;
    why = "xz: corrupt container";
    struct Rec { uint64_t unpadded, usize; };
    struct Stream { uint64_t start, index_at; uint32_t check; std::vector<Rec> recs; };
    std::vector<Stream> streams; // last first
    uint64_t end = n;
    if (n == 0) return kXzPlanFormat;
    while (end > 0) {
        // Stream Padding behind the Stream, four zero bytes at a time
        while (end >= 4 && xz_le32(p + end - 4) == 0) end -= 4;
        if (end == 0) return kXzPlanFormat; // nothing but padding, or padding in front of the first Stream
        if (end < 32) return kXzPlanFormat; // header 12 + index 8 + footer 12
        const uint8_t* f = p + end - 12;
        if (f[10] != 'Y' || f[11] != 'Z') return kXzPlanFormat;
        if (xz_crc32(f + 4, 6) != xz_le32(f)) return kXzPlanFormat;
        if (f[8] != 0 || (f[9] & 0xf0)) return kXzPlanFormat; // (reserved flag bits: liblzma answers OPTIONS_ERROR)
        Stream s;
        s.check = f[9] & 0x0f;
        const uint64_t isize = ((uint64_t)xz_le32(f + 4) + 1) * 4;
        if (isize > end - 12 - 12) return kXzPlanFormat;
        s.index_at = end - 12 - isize;
        // the Index
        const uint64_t ie = end - 12 - 4;
        if (xz_crc32(p + s.index_at, isize - 4) != xz_le32(p + ie)) return kXzPlanFormat;
        uint64_t q = s.index_at;
        if (p[q++] != 0) return kXzPlanFormat;
        uint64_t count;
        if (!xz_vli(p, &q, ie, &count) || count > isize / 2) return kXzPlanFormat;
        uint64_t blocks_len = 0;
        s.recs.reserve((size_t)count);
        for (uint64_t i = 0; i < count; ++i) {
            Rec r;
            if (!xz_vli(p, &q, ie, &r.unpadded) || !xz_vli(p, &q, ie, &r.usize)) return kXzPlanFormat;
            if (r.unpadded < 5 || r.unpadded > (1ull << 62)) return kXzPlanFormat;
            blocks_len += (r.unpadded + 3) & ~3ull;
            if (blocks_len > s.index_at) return kXzPlanFormat;
            s.recs.push_back(r);
        }
        if (ie - q > 3) return kXzPlanFormat;
        for (; q < ie; ++q)
            if (p[q]) return kXzPlanFormat;
        if (s.index_at < 12 + blocks_len) return kXzPlanFormat;
        s.start = s.index_at - blocks_len - 12;
        // the Stream header
        const uint8_t* h = p + s.start;
        static const uint8_t magic[6] = {0xFD, '7', 'z', 'X', 'Z', 0};
        if (memcmp(h, magic, 6) != 0 || xz_crc32(h + 6, 2) != xz_le32(h + 8)) return kXzPlanFormat;
        if (h[6] != f[8] || h[7] != f[9]) return kXzPlanFormat;
        end = s.start;
        streams.push_back(std::move(s));
    }
    // forward: every Block header against its record
    uint64_t out_off = 0;
    for (size_t k = streams.size(); k-- > 0;) {
        const Stream& s = streams[k];
        if (s.check != kXzCheckNone && s.check != kXzCheckCrc32 && s.check != kXzCheckCrc64 && s.check != kXzCheckSha256) {
            char b[48];
            snprintf(b, sizeof b, "xz: unsupported check %u", s.check);
            why = b;
            return kXzPlanUnsupported;
        }
        const uint64_t csz = xz_check_size(s.check);
        uint64_t at = s.start + 12;
        for (const Rec& r : s.recs) {
            uint64_t hdr = 0, hc = 0, hu = 0;
            uint32_t dict = 0;
            uint32_t bcj = 0, bcj_start = 0;
            XzBlock b;
            const int e = xz_block_header(p, at, s.index_at, &hdr, &hc, &hu, &dict, why, chains, &bcj, &bcj_start, &b);
            if (e) return e;
            if (r.unpadded < hdr + csz + 1) return kXzPlanFormat;
            b.in_off = at + hdr;
            b.in_len = r.unpadded - hdr - csz;
            b.out_off = out_off;
            b.out_len = r.usize;
            b.check = s.check;
            b.dict_size = dict;
            b.bcj = bcj;
            b.bcj_start = bcj_start;
            if (hc != ~0ull && hc != b.in_len) return kXzPlanFormat;
            if (hu != ~0ull && hu != b.out_len) return kXzPlanFormat;
            // a chunk yields at most 2 MiB and costs at least 6 bytes: a lying Index must not drive an allocation
            const uint64_t chunks = r.unpadded / 6 + 1;
            if ((b.out_len >> 21) > chunks || ((b.out_len >> 21) == chunks && (b.out_len & (kLzma2ChunkMax - 1)))) return kXzPlanFormat;
            const uint64_t padded = (r.unpadded + 3) & ~3ull; // the Block Padding lies between the data and the Check
            if (padded > s.index_at - at) return kXzPlanFormat;
            b.check_off = at + padded - csz;
            for (uint64_t z = b.in_off + b.in_len; z < b.check_off; ++z)
                if (p[z]) return kXzPlanFormat;
            at += padded;
            out_off += b.out_len;
            if (out_off > (1ull << 62)) return kXzPlanFormat;
            blocks.push_back(b);
        }
        if (at != s.index_at) return kXzPlanFormat;
    }
    *total = out_off;
    why.clear();
    return kXzPlanOk;
}

} // namespace snaphash
