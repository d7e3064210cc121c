// What tests/tar_host_harness.cpp and tests/asan_tarread.cpp share: tar_read (snappy_amd/csrc/tar_core.h) run over a heap
// buffer of exactly the stream's size, the extent invariant checked on whatever entries came back, and the mutations of the
// sweep -- every bit of a region, and every numeric header field set to four values -- each with the header's checksum as
// it was and put right again (a header whose checksum fails is refused before anything else of it is read).
#pragma once
#include <stdio.h>

#include "../snappy_amd/csrc/tar_core.h"

namespace tarsweep {

using snaphash::TarEntry;

enum : int { kInvariantBroken = 77 }; // no code of the library's (they are negative)

// every entry: data_off <= n and size <= n - data_off, without a sum that could wrap
inline bool extents_hold(const std::vector<TarEntry>& ents, uint64_t n)
{
    for (const TarEntry& e : ents)
        if (e.data_off > n || e.size > n - e.data_off) return false;
    return true;
}

// tar_read's code, or kInvariantBroken whatever the code was
inline int read_checked(const uint8_t* t, uint64_t n, std::vector<TarEntry>& ents, std::string& why)
{
    ents.clear();
    const std::vector<uint8_t> exact(t, t + n); // (no byte behind the stream may be read)
    const int rc = snaphash::tar_read(exact.data(), n, ents, why);
    return extents_hold(ents, n) ? rc : kInvariantBroken;
}

inline void fix_checksum(uint8_t* h)
{
    unsigned s = 0;
    for (int i = 0; i < 512; ++i) s += (i >= 148 && i < 156) ? ' ' : h[i];
    char f[9];
    snprintf(f, sizeof f, "%06o", s);
    memcpy(h + 148, f, 7);
    h[155] = ' ';
}

struct Sweep {
    std::vector<uint8_t> buf;
    uint64_t runs = 0;
    uint64_t broken_at = 0; // byte offset of the first mutation that broke the invariant
    std::vector<TarEntry> ents;
    std::string why;

    bool run() { ++runs; return read_checked(buf.data(), buf.size(), ents, why) != kInvariantBroken; }

    // buf with the header at h mutated by `change`: as it is, and -- unless the checksum field itself was changed -- with
    // the checksum put right; the header is restored afterwards
    template <class F> bool header_mutation(uint64_t h, bool touches_checksum, F change)
    {
        uint8_t saved[512];
        memcpy(saved, buf.data() + h, 512);
        change();
        bool ok = run();
        if (ok && !touches_checksum) {
            fix_checksum(buf.data() + h);
            ok = run();
        }
        memcpy(buf.data() + h, saved, 512);
        return ok;
    }

    // every stride-th bit of buf[off .. off+len) flipped, one at a time; header: the region is one 512-byte header block
    bool bits(uint64_t off, uint64_t len, bool header, uint64_t stride)
    {
        if (off > buf.size() || len > buf.size() - off || (header && len != 512)) return false;
        for (uint64_t b = 0; b < len * 8; b += stride) {
            const uint64_t at = off + b / 8;
            const uint8_t m = (uint8_t)(1u << (b & 7));
            bool ok;
            if (header) ok = header_mutation(off, b / 8 >= 148 && b / 8 < 156, [&] { buf[at] ^= m; });
            else { buf[at] ^= m; ok = run(); buf[at] ^= m; }
            if (!ok) { broken_at = at; return false; }
        }
        return true;
    }

    // every numeric field of the header at h set to 0, all '7', all 0xff and 0x80 + zeros
    bool fields(uint64_t h)
    {
        if (h > buf.size() || buf.size() - h < 512) return false;
        static const struct { int off, w; } kFields[] = {{100, 8}, {108, 8}, {116, 8}, {124, 12}, {136, 12}, {148, 8}};
        for (const auto& f : kFields)
            for (int v = 0; v < 4; ++v) {
                const bool ok = header_mutation(h, f.off == 148, [&] {
                    memset(buf.data() + h + f.off, v == 1 ? '7' : v == 2 ? 0xff : 0, (size_t)f.w);
                    if (v == 3) buf[h + f.off] = 0x80;
                });
                if (!ok) { broken_at = h + f.off; return false; }
            }
        return true;
    }
};

} // namespace tarsweep
