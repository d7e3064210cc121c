// Host harness of the data.tar.bz2 decoder (snappy_amd/csrc/bzip2_core.h + bzip2_host.cpp): the one-core decode, the
// block-parallel decode on host threads (from its own scan or from a given candidate list), the scan and the chain's
// block starts, for tests/test_bzip2_host.py.  Built with -DBH_MAIN it is a program that decodes mutated copies of a
// stream (run under ASan + UBSan by the same test).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "../include/snaphash.h"
#include "../snappy_amd/csrc/bzip2_host.cpp"

using namespace snaphash;

static void* give(const std::vector<uint8_t>& v, size_t* len)
{
    void* p = malloc(v.size() + 1);
    if (!v.empty()) memcpy(p, v.data(), v.size());
    *len = v.size();
    return p;
}

extern "C" {

void* bh_serial(const uint8_t* in, size_t n, size_t* len, int* rc, uint64_t* blocks)
{
    std::vector<uint8_t> out;
    *blocks = 0;
    *rc = bzip2_serial(in, n, out, blocks);
    return give(out, len);
}

void* bh_threads(const uint8_t* in, size_t n, unsigned threads, size_t* len, int* rc, uint64_t* blocks)
{
    std::vector<uint8_t> out;
    *blocks = 0;
    *rc = bzip2_host_threads(in, n, out, threads, blocks);
    return give(out, len);
}

// the decode on host threads from the candidate list cand[0..nc) (ascending)
void* bh_link(const uint8_t* in, size_t n, const uint64_t* cand, size_t nc, unsigned threads, size_t* len, int* rc)
{
    std::vector<uint8_t> out;
    std::vector<uint64_t> c(cand, cand + nc);
    uint64_t blocks = 0;
    *rc = bzip2_link_host(in, n, c, out, threads, &blocks);
    return give(out, len);
}

// the scan: up to cap candidates into out, returns how many there are
uint64_t bh_candidates(const uint8_t* in, size_t n, size_t cap, uint64_t* out)
{
    std::vector<uint64_t> c;
    const uint64_t total = bz_candidates(in, n, cap, 4, c);
    for (size_t i = 0; i < c.size(); ++i) out[i] = c[i];
    return total;
}

// the block start bits the serial decode walks through (up to cap); the number of blocks, or a negative status
int64_t bh_chain(const uint8_t* in, size_t n, uint64_t* out, size_t cap)
{
    BzCursor c;
    c.in = in;
    c.n = n;
    if (bz_cursor_stream(c, 0)) return SNAPHASH_EFORMAT;
    BzScratch s;
    std::vector<uint8_t> sink;
    int64_t k = 0;
    for (;;) {
        const int q = bz_cursor_next(c);
        if (q <= 0) return q < 0 ? q : k;
        if ((size_t)k < cap) out[k] = c.bit;
        ++k;
        sink.clear();
        const BzBlockRes r = bz_block_host(in, n, c.bit, c.level * 100000u, s, sink);
        if (r.status != kBzOk) return SNAPHASH_EFORMAT;
        bz_cursor_take(c, r.end_bit, r.crc);
    }
}

uint32_t bh_crc(const uint8_t* p, size_t n) { return bz_crc_block(p, n); }

// The BWT bytes and origPtr of the block at `bit` (the symbol stage alone, cap kBzMaxBlock): its symbol count, or a
// negative status.
int64_t bh_block_bwt(const uint8_t* in, size_t n, uint64_t bit, uint8_t* bwt, uint32_t* orig_ptr)
{
    std::unique_ptr<BzTables> t(new BzTables);
    const BzBlockRes r = bz_block_symbols(in, n, bit, bwt, kBzMaxBlock, nullptr, *t);
    *orig_ptr = r.orig_ptr;
    return r.status == kBzOk ? (int64_t)r.n : -(int64_t)r.status;
}

static void counts_of(const uint8_t* bwt, uint32_t n, uint32_t* counts)
{
    for (uint32_t c = 0; c < 256; ++c) counts[c] = 0;
    for (uint32_t i = 0; i < n; ++i) counts[bwt[i]]++;
}

// bz_ibwt: the serial walk of n steps from origPtr (1 <= n <= kBzMaxBlock, orig_ptr < n)
void bh_ibwt(const uint8_t* bwt, uint32_t n, uint32_t orig_ptr, uint8_t* out)
{
    uint32_t counts[256];
    counts_of(bwt, n, counts);
    std::vector<uint32_t> tt(n);
    bz_ibwt(bwt, n, counts, orig_ptr, tt.data(), out);
}

// The kernels' inverse BWT (bz_ibwt_kernel) with its lanes run one after another: the T vector as bz_ibwt builds it,
// the samples marked, every sample's piece walked, the pieces of origPtr's cycle linked and written, the cycle copied on
// to n bytes.  Returns 0, or kBzBad where the kernel would refuse the block; *cycle: the linked cycle's length.
int bh_ibwt_sampled(const uint8_t* bwt, uint32_t n, uint32_t orig_ptr, uint8_t* out, uint32_t* cycle)
{
    uint32_t cft[256];
    counts_of(bwt, n, cft);
    for (uint32_t c = 0, sum = 0; c < 256; ++c) {
        const uint32_t v = cft[c];
        cft[c] = sum;
        sum += v;
    }
    std::vector<uint32_t> tt(n);
    for (uint32_t i = 0; i < n; ++i) tt[cft[bwt[i]]++] = i << 8;
    const BzSamples g = bz_samples(n, orig_ptr);
    for (uint32_t j = 0; j < n; ++j) tt[j] |= bwt[j] | (bz_is_sample(g, j) ? kBzMark : 0u);
    std::vector<uint32_t> slen(kBzWalkers + 1), snext(kBzWalkers + 1), soff(kBzWalkers + 1);
    for (uint32_t s = 0; s < g.nsamp; ++s) slen[s] = bz_sample_walk(g, tt.data(), s, &snext[s]);
    const uint32_t L = bz_link_samples(g, slen.data(), snext.data(), soff.data());
    *cycle = L;
    if (!L) return kBzBad;
    for (uint32_t s = 0; s < g.nsamp; ++s)
        if (soff[s] != kBzNoPiece) bz_sample_write(g, tt.data(), s, slen[s], out + soff[s]);
    for (uint32_t k = L; k < n; ++k) out[k] = out[k % L];
    return 0;
}

void bh_free(void* p) { free(p); }

} // extern "C"

#ifdef BH_MAIN
// bh_fuzz <bz2 file> <count> <seed>: decodes `count` mutated or truncated copies of the stream, serially and on host
// threads; any out-of-bounds access or UB is the sanitizers' to report.  Prints how many decodes returned 0.
int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> bz;
    uint8_t buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) bz.insert(bz.end(), buf, buf + k);
    fclose(f);
    const long count = atol(argv[2]);
    std::mt19937_64 rng((uint64_t)atoll(argv[3]));
    long ok = 0;
    for (long it = 0; it < count; ++it) {
        std::vector<uint8_t> m = bz;
        const int kind = (int)(rng() % 4);
        if (kind == 0 && !m.empty()) {
            m.resize(rng() % m.size());
        } else {
            const int flips = 1 + (int)(rng() % 8);
            for (int q = 0; q < flips && !m.empty(); ++q) {
                const size_t at = rng() % m.size();
                if (kind == 1) m[at] ^= (uint8_t)(1u << (rng() % 8));
                else if (kind == 2) m[at] = (uint8_t)rng();
                else m.insert(m.begin() + at, (uint8_t)rng());
            }
        }
        std::vector<uint8_t> out, o2;
        uint64_t blocks = 0;
        if (bzip2_serial(m.data(), m.size(), out, &blocks) == 0) ++ok;
        if (it % 8 == 0) (void)bzip2_host_threads(m.data(), m.size(), o2, 3, &blocks);
    }
    printf("%ld\n", ok);
    return 0;
}
#endif
