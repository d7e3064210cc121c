// xz_host.cpp -- see xz_host.h.
#include "xz_host.h"

#include <string.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <thread>

#include "../../include/snaphash.h"
#include "crc_core.h"
#include "sha256_core.h"

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

} // namespace

uint64_t xz_crc64(const uint8_t* p, uint64_t n) { return ~crc64_raw_update(crc64_tab(), ~0ull, p, n); }

void xz_sha256(const uint8_t* p, uint64_t n, uint8_t* out) { sha256_host(p, n, out); }

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
    xz_chain_undo(b, out); // (the Check is over the unfiltered bytes)
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

int xz_decode_host(const uint8_t* p, size_t n, std::vector<uint8_t>& out, unsigned threads, uint64_t* nblocks, std::string& why, int chains)
{
    std::vector<XzBlock> blocks;
    uint64_t total = 0;
    const int e = xz_plan(p, n, blocks, &total, why, chains);
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
