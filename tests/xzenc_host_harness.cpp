// xzenc_host_harness.cpp -- the .xz writer's shared header (snappy_amd/csrc/xz_enc_core.h) compiled for the host, for
// tests/test_xzenc_host.py, tests/test_gpu_xzenc.py and tests/test_gpu_xzenc_edges.py: the host model of the encoder over a
// whole buffer, the operations it chose counted, every chunk's result, the model stage by stage (the arrays the three
// kernels leave in HBM), the range encoder alone over a given (probability index, bit) sequence, and xz_plan's view of a
// file.  The Checks come from the host decoder's CRC-64 (xz_host.cpp, crc_core.h).
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
    S_WATCH_BYTES = 13, S_REP0_273 = 14 /* a rep0 of 273 bytes right behind a copy of 273 */, S_MAX_DIST = 15,
    S_MAX_SLOT = 16 /* the largest distance slot of a new match */,
    S_CODED = 17 /* bytes the operations cover: all of a chunk's unless the coder gave up inside its loop */, S_N = 18
};

struct CountEncOps {
    uint64_t* s;
    uint32_t watch;
    uint32_t last_len = 0;
    void span(uint32_t pos, uint32_t len)
    {
        s[S_CODED] += len;
        if ((pos + len) % kXzEncChunk == 0) s[S_ENDS_AT_CHUNK_END]++;
        if (pos / kXzEncChunk != (pos + len - 1) / kXzEncChunk) s[S_CROSSES_CHUNK_END]++;
    }
    void lit(uint32_t matched) { s[matched ? S_MATCHED_LIT : S_LIT]++; s[S_CODED]++; last_len = 0; }
    void short_rep(uint32_t) { s[S_SHORT_REP]++; s[S_CODED]++; last_len = 0; }
    void match(uint32_t pos, uint32_t dist, uint32_t len)
    {
        s[S_MATCH]++;
        if (dist == watch) { s[S_WATCH_COUNT]++; s[S_WATCH_BYTES] += len; }
        if (dist > s[S_MAX_DIST]) s[S_MAX_DIST] = dist;
        if (lzmaenc_dist_slot(dist - 1) > s[S_MAX_SLOT]) s[S_MAX_SLOT] = lzmaenc_dist_slot(dist - 1);
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

// the operations the model chose, into stats[0 .. 18); every chunk's result into res[0 .. res_cap): the number of chunks,
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

// The model stage by stage, as the kernels leave their arrays for a piece p[0 .. n) cut into Blocks of block_size bytes:
// prev and cand (n words each, Block-relative), res and dst (a word a chunk; dst counts from out's first byte, the Blocks
// one after another), slots (kXzEncSlot bytes a chunk: the coder's output over what the caller put there) and out (chunk
// headers, bodies and every Block's end byte over what the caller put there; Block headers, padding and Checks are not
// written).  total[k]: Block k's bytes in out.  Returns the bytes of out the Blocks take, or -1 (a refused block size,
// out_cap too small).
int64_t xe_stages(const uint8_t* p, size_t n, uint64_t block_size, uint32_t* prev, uint32_t* cand, uint32_t* res, uint8_t* slots,
                  uint64_t* dst, uint8_t* out, size_t out_cap, uint64_t* total)
{
    if (!xzenc_block_size(&block_size)) return -1;
    std::vector<uint32_t> head(1u << kXzEncHashBits);
    std::vector<uint16_t> probs(kXzEncProbs);
    NoEncOps ops;
    uint64_t at = 0;
    uint32_t ch0 = 0;
    for (uint64_t b0 = 0, k = 0; b0 < n; b0 += block_size, ++k) {
        const uint32_t blen = (uint32_t)std::min<uint64_t>(block_size, n - b0);
        const uint32_t nch = (blen + kXzEncChunk - 1) / kXzEncChunk;
        uint8_t* sl = slots + (size_t)ch0 * kXzEncSlot;
        const XzEncBlockLayout L = xzenc_block_stages(p + b0, blen, prev + b0, cand + b0, head.data(), probs.data(), res + ch0, dst + ch0, sl, ops);
        if (at + L.total > out_cap) return -1;
        xzenc_block_place(p + b0, blen, res + ch0, dst + ch0, sl, out + at);
        for (uint32_t i = 0; i < nch; ++i) dst[ch0 + i] += at; // (the kernels' d_dst counts from out's first byte)
        total[k] = L.total;
        at += L.total;
        ch0 += nch;
    }
    return (int64_t)at;
}

// What the host adds to the kernels' out (xe_stages' or the device's) to make it a file: the Stream header, every
// Block's header, padding and Check, the Index and the footer.  A malloc'ed file, from the chunks' results alone.
void* xe_finish(const uint8_t* p, size_t n, uint64_t block_size, const uint32_t* res, const uint8_t* out, size_t out_len, size_t* file_len)
{
    *file_len = 0;
    if (!xzenc_block_size(&block_size)) return nullptr;
    std::vector<uint8_t> f(kXzEncStreamHeader);
    xzenc_stream_header(f.data());
    f.insert(f.end(), out, out + out_len);
    std::vector<XzEncRecord> recs;
    std::vector<uint64_t> dst;
    uint64_t at = kXzEncStreamHeader;
    uint32_t ch0 = 0;
    for (uint64_t b0 = 0; b0 < n; b0 += block_size) {
        const uint64_t blen = std::min<uint64_t>(block_size, n - b0);
        const uint32_t nch = (uint32_t)((blen + kXzEncChunk - 1) / kXzEncChunk);
        dst.resize(nch);
        const XzEncBlockLayout L = xzenc_block_layout(res + ch0, nch, blen, dst.data());
        if (at + L.total > f.size()) return nullptr;
        xzenc_block_frame(f.data() + at, L, blen, xzenc_dict_byte(block_size), xz_crc64(p + b0, blen));
        recs.push_back(XzEncRecord{L.unpadded, blen});
        at += L.total;
        ch0 += nch;
    }
    f.resize(at);
    xzenc_index_footer(recs, f);
    void* r = malloc(f.size());
    memcpy(r, f.data(), f.size());
    *file_len = f.size();
    return r;
}

// the hash of a 4-byte value (little-endian, as the chains load it)
uint32_t xe_hash(uint32_t four) { return xzenc_hash(four); }

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
