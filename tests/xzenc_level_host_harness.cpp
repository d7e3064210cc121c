// xzenc_level_host_harness.cpp -- the .xz writer's level (snappy_amd/csrc/xz_enc_core.h) compiled for the
// host, for tests/test_xzenc_level_host.py and tests/test_gpu_xzenc_level.py: the host model at a level with its lanes
// emulated in ascending or descending order, the operations it chose (counted, and one by one), the model stage by stage
// with K candidate words a position, the price table and the tables built from probabilities the caller sets.
#include <stdlib.h>
#include <string.h>

#include "../snappy_amd/csrc/xz_host.cpp"
#include "../snappy_amd/csrc/xz_enc_core.h"

using namespace snaphash;

namespace {

enum : uint32_t { T_LIT = 0, T_MATCHED_LIT = 1, T_MATCH = 2, T_REP = 3 /* +k */, T_SHORT_REP = 7, T_CROSSES_CHUNK_END = 8, T_CODED = 9, T_MAX_DIST = 10, T_N = 11 };

// counts the operations, and keeps each as (kind, position, distance or k, length): kind 0 literal, 1 short rep, 2 rep, 3 match
struct LogEncOps {
    uint64_t* s;
    uint32_t* log;
    size_t cap, n = 0;
    void put(uint32_t kind, uint32_t pos, uint32_t a, uint32_t len)
    {
        if (log && n < cap) {
            log[4 * n] = kind; log[4 * n + 1] = pos; log[4 * n + 2] = a; log[4 * n + 3] = len;
        }
        ++n;
        s[T_CODED] += len;
        if (pos / kXzEncChunk != (pos + len - 1) / kXzEncChunk) s[T_CROSSES_CHUNK_END]++;
    }
    // (positions are Block-relative; the encoder tells no position with a literal)
    void lit(uint32_t matched) { s[matched ? T_MATCHED_LIT : T_LIT]++; put(0, 0xffffffffu, matched, 1); }
    void short_rep(uint32_t pos) { s[T_SHORT_REP]++; put(1, pos, 0, 1); }
    void match(uint32_t pos, uint32_t dist, uint32_t len)
    {
        s[T_MATCH]++;
        if (dist > s[T_MAX_DIST]) s[T_MAX_DIST] = dist;
        put(3, pos, dist, len);
    }
    void rep(uint32_t pos, uint32_t k, uint32_t len) { s[T_REP + k]++; put(2, pos, k, len); }
};

uint64_t crc64_of(const uint8_t* p, uint64_t n) { return xz_crc64(p, n); }
void crc64_field(const uint8_t* p, uint64_t len, uint8_t* f) { xzenc_le64(f, xz_crc64(p, len)); }

} // namespace

extern "C" {

// K, W, the depth, the lanes
void xl_consts(uint32_t* out)
{
    out[0] = kXzEncCands;
    out[1] = kXzEncWindow;
    out[2] = kXzEncDepthHigh;
    out[3] = kXzEncLanes;
}

// the host model at a level: a malloc'ed .xz file, or *rc = -1
void* xl_encode(const uint8_t* p, size_t n, uint64_t block_size, uint32_t level, int descending, uint32_t filter, size_t* out_len, int* rc)
{
    std::vector<uint8_t> out;
    NoEncOps ops;
    *rc = xzenc_host(p, n, block_size, (uint32_t)kXzCheckCrc64, out, ops, crc64_field, nullptr, filter, level, descending != 0) ? 0 : -1;
    *out_len = *rc ? 0 : out.size();
    void* q = malloc(*out_len ? *out_len : 1);
    if (*out_len) memcpy(q, out.data(), *out_len);
    return q;
}

// the level-0 file through the plain model's own entry (what tests/xzenc_host_harness.cpp's xe_encode calls)
void* xl_encode_plain(const uint8_t* p, size_t n, uint64_t block_size, size_t* out_len, int* rc)
{
    std::vector<uint8_t> out;
    NoEncOps ops;
    *rc = xzenc_host(p, n, block_size, out, ops, crc64_of) ? 0 : -1;
    *out_len = *rc ? 0 : out.size();
    void* q = malloc(*out_len ? *out_len : 1);
    if (*out_len) memcpy(q, out.data(), *out_len);
    return q;
}

void xl_free(void* p) { free(p); }

// The operations the model chose: counted into stats[0 .. 11), every chunk's result into res[0 .. res_cap), and -- log
// != null -- each as four words into log[0 .. 4 * log_cap).  *n_ops: how many there were.  Returns the chunks, or -1.
int64_t xl_ops(const uint8_t* p, size_t n, uint64_t block_size, uint32_t level, int descending, uint64_t* stats, uint32_t* res, size_t res_cap,
               uint32_t* log, size_t log_cap, uint64_t* n_ops)
{
    std::vector<uint8_t> out;
    for (uint32_t i = 0; i < T_N; ++i) stats[i] = 0;
    LogEncOps ops{stats, log, log_cap};
    XzEncInfo info;
    if (!xzenc_host(p, n, block_size, (uint32_t)kXzCheckCrc64, out, ops, crc64_field, &info, 0, level, descending != 0)) return -1;
    for (size_t i = 0; i < info.res.size() && i < res_cap; ++i) res[i] = info.res[i];
    *n_ops = ops.n;
    return (int64_t)info.res.size();
}

// xe_stages (tests/xzenc_host_harness.cpp) at a level: cand holds K words a position at level 1
int64_t xl_stages(const uint8_t* p, size_t n, uint64_t block_size, uint32_t level, uint32_t* prev, uint32_t* cand, uint32_t* res, uint8_t* slots,
                  uint64_t* dst, uint8_t* out, size_t out_cap, uint64_t* total)
{
    if (!xzenc_block_size(&block_size) || level > kXzEncLevelMax) return -1;
    const uint32_t kw = level ? kXzEncCands : 1;
    std::vector<uint32_t> head(1u << kXzEncHashBits);
    std::vector<uint16_t> probs(kXzEncProbs);
    NoEncOps ops;
    uint64_t at = 0;
    uint32_t ch0 = 0;
    for (uint64_t b0 = 0, k = 0; b0 < n; b0 += block_size, ++k) {
        const uint32_t blen = (uint32_t)std::min<uint64_t>(block_size, n - b0);
        const uint32_t nch = (blen + kXzEncChunk - 1) / kXzEncChunk;
        uint8_t* sl = slots + (size_t)ch0 * kXzEncSlot;
        const XzEncBlockLayout L = xzenc_block_stages(p + b0, blen, prev + b0, cand + b0 * kw, head.data(), probs.data(), res + ch0, dst + ch0, sl, ops,
                                                      (uint32_t)kXzCheckCrc64, 0, level);
        if (at + L.total > out_cap) return -1;
        xzenc_block_place(p + b0, blen, res + ch0, dst + ch0, sl, out + at);
        for (uint32_t i = 0; i < nch; ++i) dst[ch0 + i] += at;
        total[k] = L.total;
        at += L.total;
        ch0 += nch;
    }
    return (int64_t)at;
}

// xzenc_chunk_priced alone over the Block blk[0 .. blen) as ONE chunk (blen <= 65 536), with the caller's candidates (K words
// a position, whatever they are: the tie-break tests hand it two of one length) and the caller's probabilities (probs_in:
// kXzEncProbs of them, or null for the reset state).  The operations go to log as in xl_ops; the coder's output to out[0 ..
// kXzEncSlot).  Returns the chunk's result.
uint32_t xl_chunk(const uint8_t* blk, uint32_t blen, const uint32_t* cand, const uint16_t* probs_in, int descending, uint8_t* out, uint32_t* log,
                  size_t log_cap, uint64_t* n_ops)
{
    std::vector<uint16_t> probs(kXzEncProbs, (uint16_t)kLzmaProbInit);
    if (probs_in) memcpy(probs.data(), probs_in, kXzEncProbs * sizeof(uint16_t));
    std::vector<XzEncWork> w(1);
    uint64_t stats[T_N] = {0};
    LogEncOps ops{stats, log, log_cap};
    XzEncHostLanes ln{descending != 0};
    const uint32_t r = xzenc_chunk_priced(blk, 0, blen, cand, probs.data(), w[0], out, kXzEncSlot, ops, ln);
    *n_ops = ops.n;
    return r;
}

// the bit-price table: 128 entries, entry i for the probabilities 16 i .. 16 i + 15
void xl_price_table(uint16_t* out)
{
    for (uint32_t i = 0; i < 128; ++i) out[i] = (uint16_t)xzenc_price_of(16 * i + 8);
}

// The tables as xzenc_chunk_priced builds them, from the caller's probabilities (kXzEncProbs of them): lenp[2][4][272],
// slotp[4][44], alignp[16]; and what the routines that read them give: a distance's price behind each length 2..9 for every
// distance of dists[0 .. nd), into distp[nd][8], and a literal's price at position 1 of the two bytes lit[0 .. 2) in
// state 0 and -- against the byte itself as the match byte -- in state 7, into litp[2].
void xl_tables(const uint16_t* probs, uint16_t* lenp, uint16_t* slotp, uint16_t* alignp, const uint32_t* dists, size_t nd, uint32_t* distp,
               const uint8_t* lit, uint32_t* litp)
{
    std::vector<XzEncWork> w(1);
    xl_price_table(w[0].ptab);
    for (uint32_t i = 0; i < kXzEncTableEntries; ++i) xzenc_table_entry(w[0], probs, i);
    memcpy(lenp, w[0].lenp, sizeof w[0].lenp);
    memcpy(slotp, w[0].slotp, sizeof w[0].slotp);
    memcpy(alignp, w[0].alignp, sizeof w[0].alignp);
    for (size_t i = 0; i < nd; ++i)
        for (uint32_t len = 2; len < 10; ++len) distp[8 * i + len - 2] = xzp_dist(w[0], probs, dists[i] - 1, len);
    litp[0] = xzp_literal(w[0].ptab, probs, lit, 1, 0, 0);
    litp[1] = xzp_literal(w[0].ptab, probs, lit, 1, 7, 0);
}

// xzenc_find_set at position p of the Block blk[0 .. blen), in the chunk that ends at ce: K words into out
void xl_find_set(const uint8_t* blk, uint32_t blen, uint32_t p, uint32_t ce, uint32_t* out)
{
    std::vector<uint32_t> prev(blen), head(1u << kXzEncHashBits);
    xzenc_chains_host(blk, blen, prev.data(), head.data());
    xzenc_find_set(blk, prev.data(), p, ce, out);
}

} // extern "C"
