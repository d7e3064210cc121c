// lzma2_check_core.h -- the .xz producer's self-check: does an LZMA2 chunk decode to exactly the bytes it
// was made from?  Shared by lzma2_check_kernel (lzma2_check_kernels.hip), a host harness in tests/ and a sanitizer program,
// the way deflate_check_core.h serves the DEFLATE producer: one walk, compiled for host and device.
//
// The producer cuts the staged stream `in` into Blocks of block_size bytes and every Block into chunks of kLzCheckChunk
// bytes; every chunk resets the coder state and carries its properties (0xE0 / 0xC0, or 0x01 / 0x02 for a stored chunk)
// and keeps the Block's dictionary (xz_enc_core.h).  So chunk c owns one stretch z[zb .. ze) of the compressed bytes and
// can be walked on its own -- by a checker, not by a decoder: a decoder needs the earlier chunks' output as its
// dictionary, the checker has the staged input, which is what that output must be.  lzma2_check_walk runs xz_core.h's
// lzma_run over the stretch and WRITES NOTHING: a literal (put) is compared with the staged byte it stands for, a match
// (length, distance) with the staged stream itself -- in[p .. p+len) against in[p-dist .. p-dist+len), what a decoder would
// copy if everything before p decoded right, and everything before p has been compared already (by this walk, or by the
// walks of the Block's earlier chunks: a Block is good when all its chunks are accepted).  The literal after a match
// reads its match byte from the staged stream (out_at).
//
// A chunk is accepted when
//   - its header is the producer's form: the first chunk of a Block 0xE0|.. with properties 0x5D (lc=3 lp=0 pb=2) or 0x01,
//     a later one 0xC0|.. with 0x5D or 0x02 (anything else is refused, not handled: the probabilities are sized for 0x5D);
//   - the header's uncompressed size is the chunk's length;
//   - header plus compressed size, plus the LZMA2 end byte 0x00 behind a Block's LAST chunk, is exactly the stretch;
//   - the coder ends as lzma2_blocks_kernel demands: every compressed byte consumed and code == 0;
//   - every byte compared equal.
// Every path is bounded as in lzma_run: the IO gives zeros past the stretch's end and remembers it, and the walk ends at
// the next symbol.  `in` is read only inside [start of the chunk's Block, end of the chunk), z only inside [zb, ze).
#pragma once
#include <stdint.h>

#include "xz_core.h"

namespace snaphash {

constexpr uint32_t kLzCheckChunk = 65536;                      // input bytes per chunk: the producer's (xz_enc_core.h kXzEncChunk)
constexpr uint32_t kLzCheckProbs = kLzmaLitBase + (0x300u << 3); // lc=3 lp=0: 7 990 probabilities, 15 980 bytes
constexpr uint32_t kLzCheckProps = 0x5D;

enum : uint32_t {
    kLzCheckOk = 0,
    kLzCheckLiteral = 1,  // a literal (or a stored byte) is not the staged byte at `offset`
    kLzCheckMatch = 2,    // a match's or a short rep's copy differs from the staged stream at `offset`
    kLzCheckDistance = 3, // a distance beyond the bytes in front of the position in its Block (or block_size)
    kLzCheckBad = 4,      // not the producer's LZMA2: control byte, properties, dictionary reset inside a Block, first
                          // range coder byte not zero, end marker, input overrun
    kLzCheckLong = 5,     // a match longer than what is left of the chunk
    kLzCheckUsize = 6,    // the header's uncompressed size is not the chunk's
    kLzCheckEnd = 7,      // sizes or the coder's end do not meet the stretch's end (a missing, non-zero or misplaced end byte too)
    kLzCheckTable = 8,    // the chunk's table entry lies outside the compressed bytes, or z_end < z_beg (nothing was read)
};

struct Lzma2Verdict {
    uint32_t status; // kLzCheck*
    uint32_t offset; // within the chunk: the first byte that differs, else how far the walk had come
};
XZ_HD Lzma2Verdict lz_verdict(uint32_t status, uint64_t offset) { return Lzma2Verdict{status, (uint32_t)offset}; }

// where chunk c of in[0 .. n_in) lies, with Blocks of bs bytes (a multiple of kLzCheckChunk)
struct Lzma2CheckPlace {
    uint64_t p0, blk0; // the chunk's and its Block's first byte
    uint32_t len;
    bool first, last;  // of its Block
};
XZ_HD Lzma2CheckPlace lzma2_check_place(uint64_t n_in, uint64_t bs, uint32_t c)
{
    Lzma2CheckPlace pl;
    pl.p0 = (uint64_t)c * kLzCheckChunk;
    pl.blk0 = pl.p0 / bs * bs;
    const uint64_t left = n_in - pl.p0, blk_end = n_in - pl.blk0 < bs ? n_in : pl.blk0 + bs;
    pl.len = (uint32_t)(left < kLzCheckChunk ? left : kLzCheckChunk);
    pl.first = pl.p0 == pl.blk0;
    pl.last = pl.p0 + pl.len == blk_end;
    return pl;
}

// The host's IO (the kernel's fetches the compressed bytes sixteen at a time, and is otherwise this).  z and in: the two
// whole buffers; next() reads z[ip .. iend), zeros past it.  put compares, and stops the walk at the first difference
// (over() then ends lzma_run before the next symbol).
struct Lzma2CheckIO {
    const uint8_t* z;
    const uint8_t* in;
    uint64_t ip, iend;
    uint64_t diff_at;
    bool ov, diff;
    uint32_t next()
    {
        if (ip < iend) return z[ip++];
        ov = true;
        return 0;
    }
    bool over() const { return ov || diff; }
    uint32_t out_at(uint64_t p) const { return in[p]; }
    void put(uint64_t p, uint32_t b)
    {
        if (!ov && !diff && in[p] != (uint8_t)b) {
            diff = true;
            diff_at = p;
        }
    }
    uint32_t in_at(uint64_t p) const { return z[p]; }
};

// How the host takes the walk's steps: one thread, everything in order.  (The kernel's: lane 0 runs the coder, the wave
// resets the probabilities and compares.)
struct Lzma2CheckHostWalk {
    void reset(uint16_t* probs)
    {
        for (uint32_t i = 0; i < kLzCheckProbs; ++i) probs[i] = (uint16_t)kLzmaProbInit;
    }
    template <class IO> bool start(LzmaDec& d, IO& io) { return lzma_rc_start(d, io); }
    template <class IO>
    int run(LzmaDec& d, uint16_t* probs, IO& io, uint64_t& pos, uint64_t& dpos, uint64_t chunk_end, uint32_t* dist, uint32_t* len)
    {
        NoOps ops;
        return lzma_run(d, probs, io, pos, dpos, chunk_end, dist, len, ops);
    }
    // the first i with a[i] != b[i], or n
    uint32_t differ(const uint8_t* a, const uint8_t* b, uint32_t n)
    {
        for (uint32_t i = 0; i < n; ++i)
            if (a[i] != b[i]) return i;
        return n;
    }
};

// The stretch's header against the chunk's place: kLzCheckOk and h, or the status.
template <class IO> XZ_HD uint32_t lzma2_check_header(IO& io, uint64_t zb, uint64_t ze, const Lzma2CheckPlace& pl, Lzma2Chunk& h)
{
    const uint64_t zn = ze - zb;
    if (zn == 0) return kLzCheckEnd;
    const uint32_t ctl = io.in_at(zb);
    const uint32_t hdr = ctl == 0 ? 1 : ctl < 0x80 ? 3 : ctl >= 0xC0 ? 6 : 5;
    if (zn < hdr) return kLzCheckEnd; // the header itself runs past the stretch
    // (every LZMA chunk carries its properties; a Block's first chunk resets the dictionary)
    if (lzma2_chunk_header(io, zb, ze, pl.first, true, h)) return kLzCheckBad;
    if (h.kind == 0 || h.dict_reset != pl.first) return kLzCheckBad; // an end byte for a chunk; a reset inside the Block
    if (h.kind == 2 && (h.lc != 3 || h.lp != 0 || h.pb != 2)) return kLzCheckBad;
    if (h.usize != pl.len) return kLzCheckUsize;
    if ((uint64_t)h.hdr + h.csize + (pl.last ? 1 : 0) != zn) return kLzCheckEnd;
    if (pl.last && io.in_at(ze - 1) != 0) return kLzCheckEnd;
    return kLzCheckOk;
}

// what lzma_run's kRunError was about, from what it left behind
template <class IO> XZ_HD uint32_t lzma2_check_run_error(const LzmaDec& d, const IO& io, uint64_t dpos)
{
    if (io.ov) return kLzCheckBad;                                 // the symbols want more bytes than the chunk has
    if (io.diff) return d.state >= 7 ? kLzCheckMatch : kLzCheckLiteral; // (a literal leaves a state below 7, a short rep 9 or 11)
    if (d.rep0 == 0xffffffffu) return kLzCheckBad;                 // the end marker has no place in LZMA2
    if (d.rep0 >= dpos || d.rep0 >= d.dict_size) return kLzCheckDistance;
    return kLzCheckLong;
}

// Chunk c of in[0 .. n_in) against its stretch z[zb .. ze) of z[0 .. n_z).  probs: kLzCheckProbs entries of scratch (LDS
// on the GPU).  On the GPU every lane of the wave calls this with the same arguments; lane 0's verdict is the verdict.
template <class IO, class W>
XZ_HD Lzma2Verdict lzma2_check_walk(IO& io, W& w, const uint8_t* in, uint64_t n_in, uint64_t bs, uint64_t n_z, uint64_t zb, uint64_t ze,
                                    uint32_t c, uint16_t* probs)
{
    if (zb > ze || ze > n_z || (uint64_t)c * kLzCheckChunk >= n_in) return lz_verdict(kLzCheckTable, 0);
    const Lzma2CheckPlace pl = lzma2_check_place(n_in, bs, c);
    Lzma2Chunk h;
    const uint32_t st = lzma2_check_header(io, zb, ze, pl, h);
    if (st != kLzCheckOk) return lz_verdict(st, 0);
    const uint64_t body = zb + h.hdr;
    if (h.kind == 1) { // stored: the bytes themselves
        const uint32_t i = w.differ(io.z + body, in + pl.p0, pl.len);
        return i < pl.len ? lz_verdict(kLzCheckLiteral, i) : lz_verdict(kLzCheckOk, pl.len);
    }
    LzmaDec d{};
    d.dict_size = (uint32_t)bs;
    d.lc = 3;
    d.lp_mask = 0;
    d.pb_mask = 3;
    lzma_reset_state(d);
    w.reset(probs);
    uint64_t pos = pl.p0, dpos = pl.p0 - pl.blk0;
    const uint64_t chunk_end = pos + pl.len;
    d.prev = dpos ? in[pos - 1] : 0;
    io.ip = body;
    io.iend = body + h.csize;
    io.ov = io.diff = false;
    io.diff_at = 0;
    if (!w.start(d, io)) return lz_verdict(kLzCheckBad, 0);
    for (;;) {
        uint32_t dist = 0, len = 0;
        const int r = w.run(d, probs, io, pos, dpos, chunk_end, &dist, &len);
        if (r == kRunChunkEnd) break;
        if (r == kRunError) return lz_verdict(lzma2_check_run_error(d, io, dpos), (io.diff ? io.diff_at : pos) - pl.p0);
        // a match: dist <= dpos and len <= chunk_end - pos (lzma_run), so both ranges lie in [pl.blk0, chunk_end)
        const uint32_t i = w.differ(in + pos, in + pos - dist, len);
        if (i < len) return lz_verdict(kLzCheckMatch, pos - pl.p0 + i);
        pos += len;
        dpos += len;
        d.prev = in[pos - 1];
    }
    if (io.ip != io.iend || d.code != 0) return lz_verdict(kLzCheckEnd, pl.len);
    return lz_verdict(kLzCheckOk, pl.len);
}

// The walk on this thread.
inline Lzma2Verdict lzma2_check_chunk(const uint8_t* in, uint64_t n_in, uint64_t bs, const uint8_t* z, uint64_t n_z, uint64_t zb, uint64_t ze,
                                      uint32_t c, uint16_t* probs)
{
    Lzma2CheckIO io{z, in, 0, 0, 0, false, false};
    Lzma2CheckHostWalk w;
    return lzma2_check_walk(io, w, in, n_in, bs, n_z, zb, ze, c, probs);
}

// Chunk c's stretch from the Block layouts, as the producer's host side knows them: the next chunk's place, or -- for a
// Block's last chunk -- the end of the Block's LZMA2 data (data_end: behind its end byte).  Not from the chunk headers.
inline uint64_t lzma2_check_stretch_end(const uint64_t* dst, uint32_t i, uint32_t cn, uint64_t data_end) { return i + 1 < cn ? dst[i + 1] : data_end; }

// last_error's words for a refused chunk: block and chunk count through the whole stream, at = the byte of the tar stream
inline std::string lzma2_check_error_text(const char* member, uint64_t block, uint64_t chunk, uint32_t status, uint64_t at)
{
    return std::string("self-check: ") + member + ": Block " + std::to_string(block) + ", chunk " + std::to_string(chunk) +
           " does not decode to the bytes it was made from (status " + std::to_string(status) + ") at offset " + std::to_string(at) +
           " of the tar stream";
}

} // namespace snaphash
