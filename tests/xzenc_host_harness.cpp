// xzenc_host_harness.cpp -- the .xz writer's shared header (snappy_amd/csrc/xz_enc_core.h) compiled for the host, for
// tests/test_xzenc_host.py and tests/test_gpu_xzenc.py: the host model of the encoder over a whole buffer, the operations
// it chose counted, every chunk's result, the range encoder alone over a given (probability index, bit) sequence, and
// xz_plan's view of a file.  The Checks come from the host decoder's CRC-64 (xz_host.cpp, crc_core.h).
#include <stdlib.h>
#include <string.h>

#include "../snappy_amd/csrc/xz_host.cpp"
#include "../snappy_amd/csrc/xz_enc_core.h"

using namespace snaphash;

namespace {

// the statistics' layout (test_xzenc_host.py names the same offsets)
enum : uint32_t {
    S_LIT = 0, S_MATCHED_LIT = 1, S_MATCH = 2, S_REP = 3 /* +k */, S_SHORT_REP = 7, S_ENDS_AT_CHUNK_END = 8 /* a match or rep whose last byte
    is a chunk's last */, S_CROSSES_CHUNK_END = 9, S_CHUNKS = 10, S_STORED = 11, S_WATCH_COUNT = 12 /* new matches of the watched distance */,
    S_WATCH_BYTES = 13, S_REP0_273 = 14 /* a rep0 of 273 bytes right behind a copy of 273 */, S_MAX_DIST = 15, S_N = 16
};

struct CountEncOps {
    uint64_t* s;
    uint32_t watch;
    uint32_t last_len = 0;
    void span(uint32_t pos, uint32_t len)
    {
        if ((pos + len) % kXzEncChunk == 0) s[S_ENDS_AT_CHUNK_END]++;
        if (pos / kXzEncChunk != (pos + len - 1) / kXzEncChunk) s[S_CROSSES_CHUNK_END]++;
    }
    void lit(uint32_t matched) { s[matched ? S_MATCHED_LIT : S_LIT]++; last_len = 0; }
    void short_rep(uint32_t) { s[S_SHORT_REP]++; last_len = 0; }
    void match(uint32_t pos, uint32_t dist, uint32_t len)
    {
        s[S_MATCH]++;
        if (dist == watch) { s[S_WATCH_COUNT]++; s[S_WATCH_BYTES] += len; }
        if (dist > s[S_MAX_DIST]) s[S_MAX_DIST] = dist;
        span(pos, len);
        last_len = len;
    }
    void rep(uint32_t pos, uint32_t k, uint32_t len)
    {
        s[S_REP + k]++;
        if (k == 0 && len == kLzmaMatchMax && last_len == kLzmaMatchMax) s[S_REP0_273]++;
        span(pos, len);
        last_len = len;
    }
};

uint64_t crc64_of(const uint8_t* p, uint64_t n) { return xz_crc64(p, n); }

} // namespace

extern "C" {

// the host model: a malloc'ed .xz file, or *rc = -1 (SNAPHASH_EINVAL) for a block size outside the format decisions
void* xe_encode(const uint8_t* p, size_t n, uint64_t block_size, size_t* out_len, int* rc)
{
    std::vector<uint8_t> out;
    NoEncOps ops;
    *rc = xzenc_host(p, n, block_size, out, ops, crc64_of) ? 0 : -1;
    *out_len = *rc ? 0 : out.size();
    void* q = malloc(*out_len ? *out_len : 1);
    if (*out_len) memcpy(q, out.data(), *out_len);
    return q;
}

void xe_free(void* p) { free(p); }

// the operations the model chose, into stats[0 .. 16); every chunk's result into res[0 .. res_cap): the number of chunks,
// or -1 for a refused block size
int64_t xe_stats(const uint8_t* p, size_t n, uint64_t block_size, uint32_t watch_dist, uint64_t* stats, uint32_t* res, size_t res_cap)
{
    std::vector<uint8_t> out;
    for (uint32_t i = 0; i < S_N; ++i) stats[i] = 0;
    CountEncOps ops{stats, watch_dist};
    XzEncInfo info;
    if (!xzenc_host(p, n, block_size, out, ops, crc64_of, &info)) return -1;
    stats[S_CHUNKS] = info.chunks;
    stats[S_STORED] = info.stored;
    for (size_t i = 0; i < info.res.size() && i < res_cap; ++i) res[i] = info.res[i];
    return (int64_t)info.res.size();
}

// The range encoder alone: bit i coded with the probability idx[i] (all start at 1024), or -- idx[i] == 0xffffffff -- as
// a direct bit; then the flush.  The bytes go to out[0 .. cap); the count is returned.
uint32_t xe_rc(const uint32_t* idx, const uint8_t* bits, size_t n, uint8_t* out, uint32_t cap)
{
    std::vector<uint16_t> probs(kXzEncProbs, (uint16_t)kLzmaProbInit);
    XzRcEnc r;
    xzrc_init(r, out, cap);
    for (size_t i = 0; i < n; ++i) {
        if (idx[i] == 0xffffffffu) xzrc_direct(r, bits[i], 1);
        else xzrc_bit(r, probs.data() + idx[i], bits[i]);
    }
    return xzrc_finish(r);
}

// xz_plan's verdict: the number of Blocks, each as (in_off, in_len, out_len, check_off, dict_size) in rec[5 * i ..], or
// -1.  (xz_plan holds every Block header's sizes against its Index record.)
int64_t xe_plan(const uint8_t* z, size_t n, uint64_t* rec, size_t cap)
{
    std::vector<XzBlock> blocks;
    uint64_t total = 0;
    std::string why;
    if (xz_plan(z, n, blocks, &total, why)) return -1;
    for (size_t i = 0; i < blocks.size() && i < cap; ++i) {
        rec[5 * i] = blocks[i].in_off;
        rec[5 * i + 1] = blocks[i].in_len;
        rec[5 * i + 2] = blocks[i].out_len;
        rec[5 * i + 3] = blocks[i].check_off;
        rec[5 * i + 4] = blocks[i].dict_size;
    }
    return (int64_t)blocks.size();
}

uint32_t xe_dict_byte(uint64_t block_size) { return xzenc_dict_byte(block_size); }

} // extern "C"
