// inflate_host.h -- the host half of the install side: gzip framing (RFC 1952), the one-core
// decoder of a whole stream, the host decode of a stretch the GPU does not take, and the segmented decode on host
// threads.  Internal; the public entry points are snaphash_gunzip_buffer / snaphash_tar_unpack (include/snaphash.h).
//
// The reference reads data.tar.gz with Go's compress/gzip (clickdeb/deb.go:427): every member of a multi-member
// stream in turn, each member's CRC-32 and ISIZE checked, FHCRC checked when present, anything after the last member
// that is not another member an error.  The same rules here; every violation is SNAPHASH_EFORMAT.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "inflate_core.h"

namespace snaphash {

// The member header at p[0..n): 0 and *hdr_len, or SNAPHASH_EFORMAT (not a gzip header, reserved flags, truncated,
// FHCRC that does not match).
int gzip_header(const uint8_t* p, size_t n, size_t* hdr_len);

// The 8-byte trailer after a member's DEFLATE stream that ended at end_bit: checks CRC-32 and ISIZE of the member's
// output, sets *next to the byte after it.  0 or SNAPHASH_EFORMAT.
int gzip_trailer(const uint8_t* p, size_t n, uint64_t end_bit, uint32_t crc, uint64_t out_len, size_t* next);

// One core, one pass: every member of gz[0..n) appended to out.  0 or SNAPHASH_EFORMAT.
int gunzip_serial(const uint8_t* gz, size_t n, std::vector<uint8_t>& out);

// The host decode of one stretch: in[0..n) from start_bit, appended to out, whose bytes from member_start on are the
// member's output so far (the window).  stop_at_flush, block_min: as inflate_run (block mode is never cut short here: the
// output buffer grows as needed).
InflateRun inflate_host_append(const uint8_t* in, size_t n, uint64_t start_bit, std::vector<uint8_t>& out, size_t member_start,
                               bool stop_at_flush, uint64_t block_min = kInfNoBlockStop);

// Byte offsets that follow the bytes 00 00 FF FF in in[0..n): where a segment may start (the LEN/NLEN of an empty
// stored block; false ones -- the same bytes inside stored data -- fall out when the segments are linked).
std::vector<uint64_t> flush_candidates(const uint8_t* in, size_t n);

// Holes of one segment (kInfHole + w in seg[0..hole_end)) filled from the bytes before it: the segment starts at
// out_base[0], and out_base[-w] is the byte w before it, for w <= avail.  false: a hole reaches past avail.
bool fill_holes_host(const uint16_t* seg, size_t len, uint8_t* out_base, size_t avail);

// The segmented decode on the host: the raw DEFLATE stream in[0..n) cut at the byte offsets starts[] (starts[0] = 0,
// ascending), every segment decoded on its own in hole mode on `threads` host threads, then linked (each one must end
// where the next starts, the last with the final block) and its holes filled in order; the bytes are appended to out.
// 0 or SNAPHASH_EFORMAT; *end_bit: where the final block ended.
int inflate_segments_host(const uint8_t* in, size_t n, const uint64_t* starts, size_t nstarts, std::vector<uint8_t>& out,
                          unsigned threads, uint64_t* end_bit);

} // namespace snaphash
