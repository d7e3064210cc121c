// sha256_host_harness.cpp -- snappy_amd/csrc/sha256_core.h compiled for the host, for tests/test_sha256_host.py and
// tests/test_gpu_xz_sha256.py: the core over a whole message, the kernel's lane routine run serially over a fetcher of
// aligned 16-byte words that counts what it is asked for, and the .xz writer's host model (xz_enc_core.h) with the Check
// of the caller's choice, its Checks from the host side (xz_host.cpp).
#include <stdlib.h>
#include <string.h>

#include "../snappy_amd/csrc/xz_host.cpp"
#include "../snappy_amd/csrc/xz_enc_core.h"

using namespace snaphash;

extern "C" {

// the units the kernel moves at a time (sha256_core.h), for the tests that walk its edges
uint32_t sh_block_bytes() { return kSha256Block; }
uint32_t sh_load_bytes() { return kSha256Load; }
uint32_t sh_step_bytes() { return kSha256Step; }
uint32_t sh_tile_row_bytes() { return kSha256TileRow; }
uint64_t sh_blocks(uint64_t len) { return sha256_blocks(len); }

void sh_sha256(const uint8_t* p, uint64_t n, uint8_t* out) { sha256_host(p, n, out); }

// The range buf[start .. start + len) as a lane of the kernel takes it, where buf stands at a 16-byte boundary: aligned
// word j is buf[16 * (start / 16 + j) ..].  fetched[j] counts the times word j was asked for (words_cap entries).  Returns
// the number of words asked for that do not overlap the range, or that lie outside fetched[].  No byte of a word that was
// not asked for is read: such words are not there (the fetcher copies from buf only what it is asked for).
uint64_t sh_lane(const uint8_t* buf, uint64_t start, uint64_t len, uint8_t* out, uint32_t* fetched, uint64_t words_cap)
{
    const uint32_t sh = (uint32_t)(start & 15);
    const uint64_t word0 = start - sh;
    uint64_t outside = 0;
    sha256_lane_serial(sh, len, out, [&](uint64_t j, uint32_t* q) {
        const uint64_t lo = word0 + 16 * j, hi = lo + 16;
        if (j >= words_cap || len == 0 || hi <= start || lo >= start + len) {
            ++outside;
            q[0] = q[1] = q[2] = q[3] = 0xdeadbeefu;
            return;
        }
        fetched[j]++;
        memcpy(q, buf + lo, 16);
    });
    return outside;
}

// the host model of the .xz writer with Check `check`: a malloc'ed file, or *rc = -1 for a refused block size or Check.
// with_check == 0: through the signature that names no Check (CRC-64)
void* sh_xz_encode(const uint8_t* p, size_t n, uint64_t block_size, uint32_t check, int with_check, size_t* out_len, int* rc)
{
    std::vector<uint8_t> out;
    NoEncOps ops;
    bool ok;
    if (!with_check) {
        ok = xzenc_host(p, n, block_size, out, ops, [](const uint8_t* q, uint64_t len) { return xz_crc64(q, len); });
    } else {
        ok = xzenc_host(p, n, block_size, check, out, ops, [&](const uint8_t* q, uint64_t len, uint8_t* f) {
            if (check == kXzCheckCrc32) xzenc_le32(f, xz_crc32(q, len));
            if (check == kXzCheckCrc64) xzenc_le64(f, xz_crc64(q, len));
            if (check == kXzCheckSha256) xz_sha256(q, len, f);
        });
    }
    *rc = ok ? 0 : -1;
    *out_len = ok ? out.size() : 0;
    void* r = malloc(*out_len ? *out_len : 1);
    if (*out_len) memcpy(r, out.data(), *out_len);
    return r;
}

void sh_free(void* p) { free(p); }

} // extern "C"
