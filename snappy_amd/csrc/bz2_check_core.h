// bz2_check_core.h -- the .bz2 producer's self-check: does a bzip2 block decode to exactly the piece of the
// staged stream it was made from?  Shared by bz2_check_kernels.hip, a host harness in tests/ and a sanitizer program, the
// way lzma2_check_core.h serves the .xz producer.
//
// The LZMA2 walker compares match by match against the staged bytes; a bzip2 block cannot be checked without undoing the
// BWT, so the check is the install side's decode (bzip2_core.h: the symbols, the inverse BWT, the RLE1 undo) with the last
// stage's store replaced by a compare.  One block at a time: its bit stretch [z_beg, z_end) of the compressed bytes
// z[0 .. n_z), its piece in[in_off .. in_off + in_len) of the staged stream in[0 .. n_in), the CRC the host holds for the
// piece, and the stream's level.  The answer is {status, offset}; nothing else is written but the decoder's scratch.
// The verdicts, in order of precedence:
//
//   status  meaning                                                                  offset
//   0       accepted                                                                 in_len
//   8       the table entry lies outside the compressed bytes, or z_end < z_beg,     0
//           or the piece lies outside the staged buffer (nothing was read)
//   3       no valid block at z_beg (magic, randomised bit, maps, selectors,         bz_block_symbols' own status
//           tables, truncated; an empty block too)                                   (2 truncated, 4 bad)
//   4       more symbols than 100 000 x level                                        the cap
//   7       origPtr >= n, or the walk breaks                                         origPtr
//   5       the block does not end at z_end                                          low 32 bits of its end_bit - z_beg
//   6       the stored block CRC is not the piece's                                  0
//   1       a byte differs                                                           the first differing byte within the piece
//   2       all of min(decoded, in_len) bytes agree and the lengths differ           that minimum
//
// The check takes any valid block, not only this producer's: six tables, 20-bit codes, any origPtr of a periodic block's
// tie group (each walks the same bytes).  Every loop is bounded by the block's symbol count n, by in_len or by a constant;
// z is read only inside [0, n_z) (bzip2_core.h's reader gives zeros past it), `in` only inside [in_off, in_off + in_len),
// however long a run expands.
#pragma once
#include <stdint.h>

#include <string>

#include "bzip2_core.h"
#include "bzip2_host.h"

namespace snaphash {

enum : uint32_t {
    kBz2CheckOk = 0,
    kBz2CheckByte = 1,    // a decoded byte is not the staged byte at `offset`
    kBz2CheckLength = 2,  // every byte both have agrees, and the block decodes to more or fewer bytes than the piece has
    kBz2CheckBlock = 3,   // no valid block at z_beg
    kBz2CheckCap = 4,     // more symbols than the level allows a block
    kBz2CheckEnd = 5,     // the block's end-of-block symbol does not end at z_end
    kBz2CheckCrc = 6,     // the stored block CRC is not the one the host holds for the piece
    kBz2CheckOrigPtr = 7, // origPtr >= n, or the inverse BWT's walk breaks
    kBz2CheckTable = 8,   // the table entry lies outside the buffers (nothing was read)
    kBz2CheckPending = 0xffffffffu, // between the link and the compare step: no early verdict.  Never a final status.
};

struct Bz2Verdict {
    uint32_t status; // kBz2Check*
    uint32_t offset;
};
BZ_HD Bz2Verdict bz2_verdict(uint32_t status, uint64_t offset) { return Bz2Verdict{status, (uint32_t)offset}; }

// one block's entry of the check's tables
struct Bz2CheckJob {
    uint64_t z_beg, z_end; // bits of z
    uint64_t in_off, in_len;
    uint32_t crc;
    uint32_t reserved;
};

BZ_HD uint32_t bz2_check_cap(uint32_t level) { return 100000u * level; } // what a decoder allows a block of a BZh<level> stream

BZ_HD bool bz2_check_table_ok(const Bz2CheckJob& j, uint64_t n_z, uint64_t n_in)
{
    return j.z_beg <= j.z_end && j.z_end / 8 + (j.z_end % 8 ? 1 : 0) <= n_z && j.in_off <= n_in && j.in_len <= n_in - j.in_off;
}

// What the symbol stage left (r; a default BzBlockRes where the table entry was refused and nothing was read) against the
// block's table entry: the early verdict, or kBz2CheckPending with B made ready for the inverse BWT and the RLE1 stages.
// Blk: bzip2_kernels.h's BzGpuBlock, or the host's stand-in with the same fields.  A block with an early verdict gets
// n = 0 and a status that is not kBzOk: bz_ibwt_kernel and bz_rle1_count_kernel skip it.
template <class Blk>
BZ_HD Bz2Verdict bz2_check_link(const BzBlockRes& r, const Bz2CheckJob& j, uint64_t n_z, uint64_t n_in, uint32_t level, uint32_t slot, Blk& B)
{
    B.out_off = 0;
    B.out_len = 0;
    B.slot = slot;
    B.n = 0;
    B.orig_ptr = r.orig_ptr;
    B.status = kBzBad;
    if (!bz2_check_table_ok(j, n_z, n_in)) return bz2_verdict(kBz2CheckTable, 0);
    if (r.status == kBzOverflow) return bz2_verdict(kBz2CheckCap, bz2_check_cap(level));
    // (bz_block_symbols sets n only once the end-of-block symbol is read: kBzBad with n > 0 is its origPtr test)
    if (r.status == kBzBad && r.n > 0) return bz2_verdict(kBz2CheckOrigPtr, r.orig_ptr);
    if (r.status != kBzOk) return bz2_verdict(kBz2CheckBlock, (uint32_t)r.status);
    if (r.end_bit != j.z_end) return bz2_verdict(kBz2CheckEnd, r.end_bit - j.z_beg);
    if (r.crc != j.crc) return bz2_verdict(kBz2CheckCrc, 0);
    B.n = r.n;
    B.status = kBzOk;
    return bz2_verdict(kBz2CheckPending, 0);
}

// The RLE1 chunks of a block of n bytes, as bz_rle1_count_kernel cuts them (bzip2_kernels.hip: at least 64 bytes, at most
// 1 024 chunks): the compare kernel reads that kernel's chunk table and must cut the same way.
BZ_HD uint32_t bz2_check_chunk_size(uint32_t n)
{
    const uint32_t cs = (n + 1023u) / 1024u;
    return cs < 64u ? 64u : cs;
}

// The compare of RLE1 bytes pre[a .. e) from state st, whose output begins at byte `pos` of the piece: the first byte that
// differs from the staged piece p[0 .. in_len), or ~0ull.  This is bz_rle1_write_kernel's loop with the store replaced by a
// compare; nothing at or beyond p + in_len is read.
BZ_HD uint64_t bz2_check_compare(BzRle1& st, const uint8_t* pre, uint32_t a, uint32_t e, uint64_t pos, const uint8_t* p, uint64_t in_len)
{
    for (uint32_t i = a; i < e && pos < in_len; ++i) {
        bool cnt;
        const uint8_t v = pre[i];
        const uint32_t m = bz_rle1_step(st, v, cnt); // at most 255
        const uint8_t b = cnt ? (uint8_t)st.last : v;
        const uint64_t room = in_len - pos;
        const uint32_t lim = m < room ? m : (uint32_t)room;
        for (uint32_t q = 0; q < lim; ++q)
            if (p[pos + q] != b) return pos + q;
        pos += m;
    }
    return ~0ull;
}

// the verdict of a block that decoded to `decoded` bytes, whose first differing byte is `first` (~0ull: none)
BZ_HD Bz2Verdict bz2_check_final(uint64_t first, uint64_t decoded, uint64_t in_len)
{
    const uint64_t m = decoded < in_len ? decoded : in_len;
    if (first < m) return bz2_verdict(kBz2CheckByte, first);
    if (decoded != in_len) return bz2_verdict(kBz2CheckLength, m);
    return bz2_verdict(kBz2CheckOk, in_len);
}

// the host's stand-in for BzGpuBlock (bzip2_kernels.h needs the runtime's headers)
struct Bz2CheckHostBlock {
    uint64_t out_off, out_len;
    uint32_t slot, n, orig_ptr;
    int32_t status;
};

// The host model, on bzip2_core.h's one-core routines: the block of table entry j, on this thread.  (bz_ibwt's walk over a
// T vector built by its own counting sort cannot break, so status 7 is the origPtr test alone here; the kernels' walk, split
// at samples, reports a broken link the same way and cannot meet one either.)
inline Bz2Verdict bz2_check_block(const uint8_t* z, uint64_t n_z, const uint8_t* in, uint64_t n_in, const Bz2CheckJob& j, uint32_t level, BzScratch& s)
{
    BzBlockRes r;
    if (bz2_check_table_ok(j, n_z, n_in)) r = bz_block_symbols(z, n_z, j.z_beg, s.bwt.data(), bz2_check_cap(level), s.counts, s.t);
    Bz2CheckHostBlock B;
    const Bz2Verdict early = bz2_check_link(r, j, n_z, n_in, level, 0, B);
    if (early.status != kBz2CheckPending) return early;
    bz_ibwt(s.bwt.data(), B.n, s.counts, B.orig_ptr, s.tt.data(), s.pre.data());
    BzRle1 st;
    const uint64_t first = bz2_check_compare(st, s.pre.data(), 0, B.n, 0, in + j.in_off, j.in_len);
    BzRle1 st2;
    const uint64_t decoded = bz_rle1(st2, s.pre.data(), B.n, nullptr, 0);
    return bz2_check_final(first, decoded, j.in_len);
}

// last_error's words for a refused block: the block counts through the whole stream, at = the byte of the tar stream
inline std::string bz2_check_error_text(const char* member, uint64_t block, uint32_t status, uint64_t at)
{
    return std::string("self-check: ") + member + ": block " + std::to_string(block) + " does not decode to the bytes it was made from (status " +
           std::to_string(status) + ") at offset " + std::to_string(at) + " of the tar stream";
}

} // namespace snaphash
