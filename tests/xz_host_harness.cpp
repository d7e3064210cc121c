// xz_host_harness.cpp -- the .xz decoder's shared header (snappy_amd/csrc/xz_core.h), the host decoder (xz_host.cpp) and
// the CRC-64 core (crc_core.h) compiled for the host, for tests/test_xz_host.py: whole files decoded, a histogram of the
// LZMA operations and LZMA2 chunks a file exercised, the kernel's wave-copy index arithmetic run lane by lane, and the
// CRC-64 arithmetic the kernels use run serially.
#include <stdlib.h>
#include <string.h>

#include "../snappy_amd/csrc/xz_host.cpp"

using namespace snaphash;

namespace {

// the histogram's layout (test_xz_host.py names the same offsets)
enum : uint32_t {
    H_LIT = 0, H_MATCHED_LIT = 1, H_MATCH = 2, H_REP = 3 /* +k */, H_SHORT_REP = 7, H_DIST_ALL = 8, H_DIST_DICT = 9,
    H_COPY = 10 /* + 4 * dist class + len class */, H_CTL = 26 /* + control byte */, H_LC = 282, H_LP = 287, H_PB = 292,
    H_CHUNK_1 = 297, H_CHUNK_2M = 298, H_CHUNK_BIG = 299 /* within 64 KiB of 2 MiB */, H_N = 300
};

struct CountOps {
    uint64_t* h;
    void lit(bool matched) { h[matched ? H_MATCHED_LIT : H_LIT]++; }
    void match() { h[H_MATCH]++; }
    void rep(int k) { h[H_REP + k]++; }
    void short_rep() { h[H_SHORT_REP]++; }
    void copy(uint32_t dist, uint32_t len, uint64_t dpos, uint32_t dict)
    {
        if (dist == dpos) h[H_DIST_ALL]++;
        if (dist == dict) h[H_DIST_DICT]++;
        const int di = dist == 1 ? 0 : dist == 63 ? 1 : dist == 64 ? 2 : dist == 65 ? 3 : -1;
        const int li = len == 2 ? 0 : len == 64 ? 1 : len == 65 ? 2 : len == 273 ? 3 : -1;
        if (di >= 0 && li >= 0) h[H_COPY + 4 * di + li]++;
    }
};

} // namespace

extern "C" {

void* xh_decode(const uint8_t* p, size_t n, unsigned threads, size_t* out_len, int* rc)
{
    std::vector<uint8_t> out;
    std::string why;
    *rc = xz_decode_host(p, n, out, threads, nullptr, why);
    *out_len = *rc ? 0 : out.size();
    void* q = malloc(out.size() ? out.size() : 1);
    if (*out_len) memcpy(q, out.data(), out.size());
    return q;
}

void xh_free(void* p) { free(p); }

// every Block of the file decoded on this thread with the operations counted into hist[0 .. 300); 0, or nonzero when the
// file does not decode
int xh_hist(const uint8_t* p, size_t n, uint64_t* hist)
{
    std::vector<XzBlock> blocks;
    uint64_t total = 0;
    std::string why;
    if (xz_plan(p, n, blocks, &total, why)) return 1;
    std::vector<uint16_t> probs(kLzmaProbsMax);
    for (const XzBlock& b : blocks) {
        std::vector<uint8_t> out(b.out_len ? b.out_len : 1);
        CountOps ops{hist};
        Lzma2Trace tr;
        if (lzma2_block_host(p + b.in_off, b.in_len, out.data(), b.out_len, b.dict_size, probs.data(), ops, &tr) != kXzOk) return 2;
        for (uint8_t c : tr.controls) hist[H_CTL + c]++;
        for (uint32_t pr : tr.props) {
            hist[H_LC + (pr & 15)]++;
            hist[H_LP + (pr >> 4 & 15)]++;
            hist[H_PB + (pr >> 8 & 15)]++;
        }
        for (uint32_t u : tr.usizes) {
            if (u == 1) hist[H_CHUNK_1]++;
            if (u == kLzma2ChunkMax) hist[H_CHUNK_2M]++;
            if (u > kLzma2ChunkMax - 65536) hist[H_CHUNK_BIG]++;
        }
    }
    return 0;
}

// The kernel's match copy (xz_copy_lane, a lane at a time, lanes in descending order to show that no lane depends on
// another) against the byte-by-byte copy, for every dist in [1, max_dist] and len in [2, max_len]: the number of (dist,
// len) pairs that differ in the body, in the byte the wave reports as its last, or that touch a byte outside the body.
uint64_t xh_copy_check(uint32_t max_dist, uint32_t max_len)
{
    uint64_t bad = 0;
    const uint32_t front = max_dist, guard = 64;
    std::vector<uint8_t> a(front + max_len + guard), b(a.size());
    for (uint32_t dist = 1; dist <= max_dist; ++dist)
        for (uint32_t len = 2; len <= max_len; ++len) {
            for (size_t i = 0; i < a.size(); ++i) a[i] = b[i] = (uint8_t)(i * 131 + dist * 7 + len + (i >> 3));
            const uint64_t pos = front;
            for (uint32_t i = 0; i < len; ++i) a[pos + i] = a[pos + i - dist];
            uint32_t last[kXzWave];
            for (uint32_t lane = kXzWave; lane-- > 0;) last[lane] = xz_copy_lane(b.data(), pos, dist, len, lane);
            if (a != b || last[(len - 1) % kXzWave] != a[pos + len - 1]) ++bad;
        }
    return bad;
}

uint64_t xh_crc64(const uint8_t* p, size_t n) { return xz_crc64(p, n); }

uint64_t xh_crc64_combine(uint64_t a, uint64_t b, uint64_t len_b)
{
    Crc64PowTable t;
    crc64_pow_table(t);
    return crc64_combine(t, a, b, len_b);
}

uint64_t xh_crc64_xpow8(uint64_t n)
{
    Crc64PowTable t;
    crc64_pow_table(t);
    return crc64_xpow8(t, n);
}

// table k, entry b
uint64_t xh_crc64_table(uint32_t k, uint32_t b)
{
    static uint64_t tab[8][256];
    static bool built = false;
    if (!built) { crc64_tables(tab); built = true; }
    return tab[k & 7][b & 255];
}

// the kernels' cut of a range, run serially: lane slices from the range's end, lane shifts, tile shifts, the fold
uint64_t xh_crc64_cut(const uint8_t* p, size_t n)
{
    static uint64_t tab[8][256];
    static bool built = false;
    if (!built) { crc64_tables(tab); built = true; }
    Crc64PowTable t;
    crc64_pow_table(t);
    uint64_t acc = 0;
    const uint64_t tiles = crc_tiles_of(n);
    for (uint64_t k = 0; k < tiles; ++k) {
        uint64_t tile = 0;
        for (uint32_t lane = 0; lane < kCrcLanes; ++lane) {
            uint64_t lo, hi;
            crc_lane_slice(n, k, lane, &lo, &hi);
            if (hi > lo) tile ^= crc64_mul(crc64_raw_update(tab, 0, p + lo, hi - lo), crc64_lane_shift(t, lane));
        }
        acc ^= crc64_mul(tile, crc64_tile_shift(t, k));
    }
    return crc64_finish(t, acc, n);
}

void xh_sha256(const uint8_t* p, size_t n, uint8_t* out) { xz_sha256(p, n, out); }

} // extern "C"
