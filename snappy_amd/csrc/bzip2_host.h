// bzip2_host.h -- the host half of the data.tar.bz2 side: the stream framing (stream headers, end-of-stream magic,
// combined CRC, concatenated streams), the one-core decoder, the scan for block starts, and the block-parallel decode on
// host threads.  Internal; the public entry points are snaphash_bunzip2_buffer / snaphash_tar_unpack_bz2
// (include/snaphash.h).
//
// The reference reads data.tar.bz2 with Go's compress/bzip2 (clickdeb/deb.go skipToArMember): every stream of a
// concatenation in turn, every block CRC and each stream's combined CRC checked, the randomised bit refused, a block
// longer than its level allows refused, anything after the last stream that is not another stream an error.  The same
// rules here; every violation is SNAPHASH_EFORMAT.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <memory>
#include <vector>

#include "bzip2_core.h"

namespace snaphash {

// Walks the stream framing around the blocks: where the next block starts, which level it has, the combined CRC.
struct BzCursor {
    const uint8_t* in = nullptr;
    uint64_t n = 0;
    uint64_t bit = 0;       // where the next block or end-of-stream magic starts
    uint32_t level = 0;     // block limit of the current stream: level x 100 000 symbols
    uint32_t combined = 0;  // the current stream's combined CRC so far
};

// The stream header at byte `at`: 0 or SNAPHASH_EFORMAT ("BZh" + a digit 1-9).
int bz_cursor_stream(BzCursor& c, uint64_t at);
// What lies at c.bit: 1 = a block magic; 0 = the input ended right after an end-of-stream (whose combined CRC matched;
// any further stream headers on the way are taken); SNAPHASH_EFORMAT for anything else.
int bz_cursor_next(BzCursor& c);
// A block that ended at end_bit with stored CRC crc (already checked against its bytes) was taken.
inline void bz_cursor_take(BzCursor& c, uint64_t end_bit, uint32_t crc)
{
    c.combined = bz_crc_combine(c.combined, crc);
    c.bit = end_bit;
}

uint32_t bz_crc_block(const uint8_t* p, uint64_t n); // a block's CRC over its output

// Scratch of one host decoder (the tables and the three block-sized buffers).
struct BzScratch {
    BzTables t;
    std::vector<uint8_t> bwt, pre;
    std::vector<uint32_t> tt;
    uint32_t counts[256];
    BzScratch() : bwt(kBzMaxBlock), pre(kBzMaxBlock), tt(kBzMaxBlock) {}
};

// One whole block on the host: the symbols (at most cap), the inverse BWT, the RLE1 undo appended to out, and its CRC
// checked (a mismatch is kBzBad).  out keeps what it held before.
BzBlockRes bz_block_host(const uint8_t* in, uint64_t n, uint64_t bit, uint32_t cap, BzScratch& s, std::vector<uint8_t>& out);

// One core, one pass: every stream of in[0..n) appended to out.  0 or SNAPHASH_EFORMAT; *blocks (may be null) += blocks.
int bzip2_serial(const uint8_t* in, size_t n, std::vector<uint8_t>& out, uint64_t* blocks);

// Bit offsets of every block magic in in[0..n), ascending, on `threads` threads; at most cap are kept, the return value
// counts them all (more than cap: the caller decodes in chain order instead).
uint64_t bz_candidates(const uint8_t* in, size_t n, size_t cap, unsigned threads, std::vector<uint64_t>& out);

// The candidate cap of an n-byte input: a real block takes at least 40-odd bytes, so this only bites on planted magics.
inline size_t bz_candidate_cap(size_t n) { return n / 32 + 64; }

// The block-parallel decode on host threads: every candidate block decoded whole (symbols, iBWT, RLE1, CRC) by
// `threads` workers a bounded distance ahead of this thread, which walks the chain from the stream header and appends
// each linked block's bytes in order; false candidates drop out.  More candidates than the cap: bzip2_serial.
// 0 or SNAPHASH_EFORMAT; *blocks += blocks decoded.
int bzip2_host_threads(const uint8_t* in, size_t n, std::vector<uint8_t>& out, unsigned threads, uint64_t* blocks);
// The same from a given candidate list (ascending bit offsets; false ones and missing ones are allowed: a chain block
// that is no candidate is decoded by the linking thread).
int bzip2_link_host(const uint8_t* in, size_t n, const std::vector<uint64_t>& cand, std::vector<uint8_t>& out, unsigned threads,
                    uint64_t* blocks);

} // namespace snaphash
