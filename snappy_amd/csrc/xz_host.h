// xz_host.h -- the host half of the data.tar.xz side: the Blocks of a planned .xz buffer (xz_core.h) decoded on host
// threads, a Block a thread, each straight to its final offset with its Check taken by the thread that decoded it; the
// host's CRC-64/XZ (slice-by-8) and the SHA-256 of sha256_core.h for Check id 10.  Internal; the public entry points are
// snaphash_unxz_buffer / snaphash_tar_unpack_xz (include/snaphash.h).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "xz_core.h"

namespace snaphash {

uint64_t xz_crc64(const uint8_t* p, uint64_t n);            // CRC-64/XZ
void xz_sha256(const uint8_t* p, uint64_t n, uint8_t* out); // 32 bytes

// The Check field of Block b (in the file p) against the Block's decoded bytes: true when it matches (or there is none).
bool xz_check_block(const uint8_t* p, const XzBlock& b, const uint8_t* bytes);

// One Block of the file p into out[0 .. b.out_len) on this thread, its filter chain undone (xz_chain_undo) and its Check included:
// kXzOk or kXzBad.
int xz_block_host(const uint8_t* p, const XzBlock& b, uint8_t* out, uint16_t* probs);

// The Blocks `which` (indices into blocks; null: all of them) on up to `threads` threads, each to out + its out_off.
// 0 or SNAPHASH_EFORMAT.
int xz_blocks_host(const uint8_t* p, const std::vector<XzBlock>& blocks, const std::vector<uint32_t>* which, uint8_t* out, unsigned threads);

// A whole .xz buffer: plan and decode.  0, SNAPHASH_EFORMAT or SNAPHASH_EINVAL (a filter chain or Check this does not
// take; why says which).  *nblocks (may be null) = the Blocks.  chains: xz_plan's (kXzChainNone / Bcj / Any).
int xz_decode_host(const uint8_t* p, size_t n, std::vector<uint8_t>& out, unsigned threads, uint64_t* nblocks, std::string& why,
                   int chains = kXzChainNone);

} // namespace snaphash
