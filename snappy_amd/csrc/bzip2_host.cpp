// bzip2_host.cpp -- see bzip2_host.h.
#include "bzip2_host.h"

#include <string.h>

#include <algorithm>
#include <atomic>
#include <thread>

#include "../../include/snaphash.h"

namespace snaphash {

namespace {

const uint32_t* crc_table()
{
    static const struct T {
        uint32_t t[256];
        T() { bz_crc_table(t); }
    } tab;
    return tab.t;
}

uint64_t be64_at(const uint8_t* in, size_t n, size_t i)
{
    uint64_t w = 0;
    if (i + 8 <= n) {
        for (int k = 0; k < 8; ++k) w = w << 8 | in[i + k];
    } else {
        for (size_t k = 0; k < 8; ++k) w = w << 8 | (i + k < n ? in[i + k] : 0);
    }
    return w;
}

} // namespace

uint32_t bz_crc_block(const uint8_t* p, uint64_t n) { return ~bz_crc_update(crc_table(), 0xffffffffu, p, n); }

int bz_cursor_stream(BzCursor& c, uint64_t at)
{
    if (at + 4 > c.n || c.in[at] != 'B' || c.in[at + 1] != 'Z' || c.in[at + 2] != 'h' || c.in[at + 3] < '1' || c.in[at + 3] > '9')
        return SNAPHASH_EFORMAT;
    c.level = (uint32_t)(c.in[at + 3] - '0');
    c.combined = 0;
    c.bit = (at + 4) * 8;
    return 0;
}

int bz_cursor_next(BzCursor& c)
{
    for (;;) {
        if (c.bit + 48 > c.n * 8) return SNAPHASH_EFORMAT;
        const uint64_t m = bz_bits48(c.in, c.n, c.bit);
        if (m == kBzBlockMagic) return 1;
        if (m != kBzEosMagic || c.bit + 80 > c.n * 8) return SNAPHASH_EFORMAT;
        BzBits b;
        bb_start(b, c.in, c.n, c.bit + 48);
        if (bb_take(b, 32) != c.combined) return SNAPHASH_EFORMAT;
        const uint64_t at = (c.bit + 80 + 7) >> 3;
        if (at == c.n) return 0;
        if (bz_cursor_stream(c, at)) return SNAPHASH_EFORMAT; // (trailing bytes that are not another stream)
    }
}

BzBlockRes bz_block_host(const uint8_t* in, uint64_t n, uint64_t bit, uint32_t cap, BzScratch& s, std::vector<uint8_t>& out)
{
    BzBlockRes r = bz_block_symbols(in, n, bit, s.bwt.data(), std::min(cap, kBzMaxBlock), s.counts, s.t);
    if (r.status != kBzOk) return r;
    bz_ibwt(s.bwt.data(), r.n, s.counts, r.orig_ptr, s.tt.data(), s.pre.data());
    BzRle1 st;
    const uint64_t len = bz_rle1(st, s.pre.data(), r.n, nullptr, 0);
    const size_t base = out.size();
    out.resize(base + (size_t)len);
    BzRle1 st2;
    (void)bz_rle1(st2, s.pre.data(), r.n, out.data() + base, len);
    if (bz_crc_block(out.data() + base, len) != r.crc) {
        out.resize(base);
        r.status = kBzBad;
    }
    return r;
}

int bzip2_serial(const uint8_t* in, size_t n, std::vector<uint8_t>& out, uint64_t* blocks)
{
    BzCursor c;
    c.in = in;
    c.n = n;
    if (bz_cursor_stream(c, 0)) return SNAPHASH_EFORMAT; // (n == 0 too, as snaphash_gunzip_buffer)
    std::unique_ptr<BzScratch> s(new BzScratch);
    for (;;) {
        const int k = bz_cursor_next(c);
        if (k <= 0) return k;
        const BzBlockRes r = bz_block_host(in, n, c.bit, c.level * 100000u, *s, out);
        if (r.status != kBzOk) return SNAPHASH_EFORMAT;
        bz_cursor_take(c, r.end_bit, r.crc);
        if (blocks) ++*blocks;
    }
}

uint64_t bz_candidates(const uint8_t* in, size_t n, size_t cap, unsigned threads, std::vector<uint64_t>& out)
{
    out.clear();
    if (n < 6) return 0;
    threads = (unsigned)std::max<size_t>(1, std::min<size_t>(threads, n >> 20));
    std::vector<std::vector<uint64_t>> part(threads);
    std::vector<uint64_t> cnt(threads, 0);
    auto work = [&](unsigned k) {
        const size_t a = n * k / threads, e = n * (k + 1) / threads;
        for (size_t i = a; i < e; ++i) {
            const uint64_t w = be64_at(in, n, i);
            for (uint32_t sh = 0; sh < 8; ++sh) {
                if (((w << sh) >> 16) != kBzBlockMagic) continue;
                const uint64_t bit = (uint64_t)i * 8 + sh;
                if (bit + 48 > (uint64_t)n * 8) continue;
                if (++cnt[k] <= cap) part[k].push_back(bit);
            }
        }
    };
    std::vector<std::thread> th;
    for (unsigned k = 1; k < threads; ++k) th.emplace_back(work, k);
    work(0);
    for (auto& t : th) t.join();
    uint64_t total = 0;
    for (unsigned k = 0; k < threads; ++k) {
        total += cnt[k];
        for (uint64_t b : part[k]) {
            if (out.size() >= cap) break;
            out.push_back(b);
        }
    }
    return total;
}

int bzip2_host_threads(const uint8_t* in, size_t n, std::vector<uint8_t>& out, unsigned threads, uint64_t* blocks)
{
    std::vector<uint64_t> cand;
    if (bz_candidates(in, n, bz_candidate_cap(n), threads, cand) > bz_candidate_cap(n) || threads <= 1 || cand.size() <= 1)
        return bzip2_serial(in, n, out, blocks);
    return bzip2_link_host(in, n, cand, out, threads, blocks);
}

int bzip2_link_host(const uint8_t* in, size_t n, const std::vector<uint64_t>& cand, std::vector<uint8_t>& out, unsigned threads,
                    uint64_t* blocks)
{
    threads = std::max(2u, threads);
    struct Slot {
        BzBlockRes r;
        std::vector<uint8_t> bytes;
        std::atomic<int> done{0};
    };
    const size_t K = cand.size();
    std::unique_ptr<Slot[]> slot(new Slot[K]);
    std::atomic<size_t> next{0}, want{0};
    const size_t ahead = threads + 2; // candidates a worker may run ahead of the one the chain waits for (memory bound)
    auto work = [&]() {
        std::unique_ptr<BzScratch> s(new BzScratch);
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= K) return;
            while (i > want.load(std::memory_order_acquire) + ahead) std::this_thread::yield();
            if (next.load(std::memory_order_relaxed) > K + ahead) return; // (the chain has ended: give up)
            slot[i].r = bz_block_host(in, n, cand[i], kBzMaxBlock, *s, slot[i].bytes);
            slot[i].done.store(1, std::memory_order_release);
        }
    };
    struct Stop {
        std::atomic<size_t>& next;
        std::atomic<size_t>& want;
        std::vector<std::thread> th;
        size_t K;
        ~Stop()
        {
            next.store(K + 1000000);
            want.store(K + 1000000);
            for (auto& t : th) if (t.joinable()) t.join();
        }
    } stop{next, want, {}, K};
    for (unsigned k = 0; k < threads - 1; ++k) stop.th.emplace_back(work);
    BzCursor c;
    c.in = in;
    c.n = n;
    if (bz_cursor_stream(c, 0)) return SNAPHASH_EFORMAT;
    std::unique_ptr<BzScratch> own; // a chain block that is no candidate (cannot happen below the cap): decoded here
    for (;;) {
        const int k = bz_cursor_next(c);
        if (k <= 0) return k;
        const auto it = std::lower_bound(cand.begin(), cand.end(), c.bit);
        BzBlockRes r;
        if (it == cand.end() || *it != c.bit) {
            if (!own) own.reset(new BzScratch);
            r = bz_block_host(in, n, c.bit, c.level * 100000u, *own, out);
        } else {
            const size_t i = (size_t)(it - cand.begin());
            want.store(i, std::memory_order_release);
            while (!slot[i].done.load(std::memory_order_acquire)) std::this_thread::yield();
            r = slot[i].r;
            if (r.status == kBzOk && r.n > c.level * 100000u) r.status = kBzBad; // longer than the level allows
            if (r.status == kBzOk) out.insert(out.end(), slot[i].bytes.begin(), slot[i].bytes.end());
            std::vector<uint8_t>().swap(slot[i].bytes);
        }
        if (r.status != kBzOk) return SNAPHASH_EFORMAT;
        bz_cursor_take(c, r.end_bit, r.crc);
        if (blocks) ++*blocks;
    }
}

} // namespace snaphash
