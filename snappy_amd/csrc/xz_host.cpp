// xz_host.cpp -- see xz_host.h.
#include "xz_host.h"

#include <string.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <thread>

#include "../../include/snaphash.h"
#include "crc_core.h"

namespace snaphash {

namespace {

const uint64_t (*crc64_tab())[256]
{
    static const struct T {
        uint64_t t[8][256];
        T() { crc64_tables(t); }
    } tab;
    return tab.t;
}

inline uint32_t rotr(uint32_t x, int k) { return x >> k | x << (32 - k); }

const uint32_t kSha256K[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
    0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
    0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
    0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
    0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
    0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

void sha256_block(uint32_t* h, const uint8_t* p)
{
    uint32_t w[64];
    for (int i = 0; i < 16; ++i) w[i] = (uint32_t)p[4 * i] << 24 | p[4 * i + 1] << 16 | p[4 * i + 2] << 8 | p[4 * i + 3];
    for (int i = 16; i < 64; ++i) {
        const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
        const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
        w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int i = 0; i < 64; ++i) {
        const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + kSha256K[i] + w[i];
        const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

} // namespace

uint64_t xz_crc64(const uint8_t* p, uint64_t n) { return ~crc64_raw_update(crc64_tab(), ~0ull, p, n); }

void xz_sha256(const uint8_t* p, uint64_t n, uint8_t* out)
{
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    uint64_t i = 0;
    for (; i + 64 <= n; i += 64) sha256_block(h, p + i);
    uint8_t tail[128] = {0};
    const uint64_t r = n - i;
    if (r) memcpy(tail, p + i, r);
    tail[r] = 0x80;
    const uint64_t tl = r < 56 ? 64 : 128;
    const uint64_t bits = n * 8;
    for (int k = 0; k < 8; ++k) tail[tl - 1 - k] = (uint8_t)(bits >> (8 * k));
    sha256_block(h, tail);
    if (tl == 128) sha256_block(h, tail + 64);
    for (int k = 0; k < 8; ++k) {
        out[4 * k] = (uint8_t)(h[k] >> 24);
        out[4 * k + 1] = (uint8_t)(h[k] >> 16);
        out[4 * k + 2] = (uint8_t)(h[k] >> 8);
        out[4 * k + 3] = (uint8_t)h[k];
    }
}

bool xz_check_block(const uint8_t* p, const XzBlock& b, const uint8_t* bytes)
{
    const uint8_t* f = p + b.check_off;
    switch (b.check) {
    case kXzCheckNone: return true;
    case kXzCheckCrc32: return xz_crc32(bytes, b.out_len) == xz_le32(f);
    case kXzCheckCrc64: return xz_crc64(bytes, b.out_len) == ((uint64_t)xz_le32(f + 4) << 32 | xz_le32(f));
    case kXzCheckSha256: {
        uint8_t d[32];
        xz_sha256(bytes, b.out_len, d);
        return memcmp(d, f, 32) == 0;
    }
    }
    return false;
}

int xz_block_host(const uint8_t* p, const XzBlock& b, uint8_t* out, uint16_t* probs)
{
    NoOps ops;
    if (lzma2_block_host(p + b.in_off, b.in_len, out, b.out_len, b.dict_size, probs, ops) != kXzOk) return kXzBad;
    return xz_check_block(p, b, out) ? kXzOk : kXzBad;
}

int xz_blocks_host(const uint8_t* p, const std::vector<XzBlock>& blocks, const std::vector<uint32_t>* which, uint8_t* out, unsigned threads)
{
    const size_t K = which ? which->size() : blocks.size();
    if (K == 0) return 0;
    // the long Blocks first: the pass ends when its slowest thread does
    std::vector<uint32_t> order(K);
    for (size_t i = 0; i < K; ++i) order[i] = which ? (*which)[i] : (uint32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return blocks[a].out_len > blocks[b].out_len; });
    std::atomic<size_t> next{0};
    std::atomic<int> bad{0};
    auto work = [&]() {
        std::unique_ptr<uint16_t[]> probs(new uint16_t[kLzmaProbsMax]);
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= K || bad.load(std::memory_order_relaxed)) return;
            const XzBlock& b = blocks[order[i]];
            if (xz_block_host(p, b, out + b.out_off, probs.get()) != kXzOk) bad.store(1);
        }
    };
    const unsigned T = (unsigned)std::min<size_t>(K, std::max(1u, threads));
    struct Join {
        std::vector<std::thread> th;
        ~Join()
        {
            for (auto& t : th)
                if (t.joinable()) t.join();
        }
    } join;
    for (unsigned k = 1; k < T; ++k) join.th.emplace_back(work);
    work();
    for (auto& t : join.th) t.join();
    return bad.load() ? SNAPHASH_EFORMAT : 0;
}

int xz_decode_host(const uint8_t* p, size_t n, std::vector<uint8_t>& out, unsigned threads, uint64_t* nblocks, std::string& why)
{
    std::vector<XzBlock> blocks;
    uint64_t total = 0;
    const int e = xz_plan(p, n, blocks, &total, why);
    if (e) return e == kXzPlanUnsupported ? SNAPHASH_EINVAL : SNAPHASH_EFORMAT;
    const size_t o0 = out.size();
    out.resize(o0 + total);
    if (nblocks) *nblocks = blocks.size();
    if (xz_blocks_host(p, blocks, nullptr, out.data() + o0, threads)) {
        out.resize(o0);
        why = "xz: corrupt block";
        return SNAPHASH_EFORMAT;
    }
    return 0;
}

} // namespace snaphash
