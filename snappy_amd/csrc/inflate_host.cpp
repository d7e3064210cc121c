// inflate_host.cpp -- see inflate_host.h.
#include "inflate_host.h"

#include <string.h>

#include <algorithm>
#include <atomic>
#include <thread>

#include "../../include/snaphash.h"
#include "tarpack.h"

namespace snaphash {

int gzip_header(const uint8_t* p, size_t n, size_t* hdr_len)
{
    // RFC 1952 sec. 2.3; Go's gzip.Reader.readHeader: ID1 ID2 CM=8, then the optional fields the flags announce
    if (n < 10 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8) return SNAPHASH_EFORMAT;
    const uint8_t flg = p[3];
    if (flg & 0xe0) return SNAPHASH_EFORMAT; // reserved bits
    size_t at = 10;
    if (flg & 4) { // FEXTRA
        if (at + 2 > n) return SNAPHASH_EFORMAT;
        const size_t xlen = p[at] | (size_t)p[at + 1] << 8;
        at += 2 + xlen;
        if (at > n) return SNAPHASH_EFORMAT;
    }
    for (int f = 8; f <= 16; f += 8) { // FNAME, then FCOMMENT: zero-terminated
        if (!(flg & f)) continue;
        const uint8_t* z = (const uint8_t*)memchr(p + at, 0, n - at);
        if (!z) return SNAPHASH_EFORMAT;
        at = (size_t)(z - p) + 1;
    }
    if (flg & 2) { // FHCRC: the low 16 bits of the CRC-32 of the header so far
        if (at + 2 > n) return SNAPHASH_EFORMAT;
        const uint32_t want = p[at] | (uint32_t)p[at + 1] << 8;
        if ((crc32_update(0, p, at) & 0xffffu) != want) return SNAPHASH_EFORMAT;
        at += 2;
    }
    *hdr_len = at;
    return 0;
}

int gzip_trailer(const uint8_t* p, size_t n, uint64_t end_bit, uint32_t crc, uint64_t out_len, size_t* next)
{
    const size_t at = (size_t)((end_bit + 7) >> 3);
    if (at + 8 > n) return SNAPHASH_EFORMAT;
    const uint32_t want_crc = p[at] | (uint32_t)p[at + 1] << 8 | (uint32_t)p[at + 2] << 16 | (uint32_t)p[at + 3] << 24;
    const uint32_t want_len = p[at + 4] | (uint32_t)p[at + 5] << 8 | (uint32_t)p[at + 6] << 16 | (uint32_t)p[at + 7] << 24;
    if (want_crc != crc || want_len != (uint32_t)out_len) return SNAPHASH_EFORMAT;
    *next = at + 8;
    return 0;
}

InflateRun inflate_host_append(const uint8_t* in, size_t n, uint64_t start_bit, std::vector<uint8_t>& out, size_t member_start,
                               bool stop_at_flush, uint64_t block_min)
{
    InflateTables t;
    const size_t base = out.size();
    // a guess at the output (DEFLATE rarely does better than 1:8 outside runs of one byte); doubled until it holds
    size_t cap = std::max<size_t>((size_t)(n - std::min<uint64_t>(n, start_bit >> 3)) * 4, 1u << 16);
    for (;;) {
        out.resize(base + cap);
        InflateRun r = inflate_run<uint8_t>(in, n, start_bit, out.data() + base, base - member_start, cap, false, stop_at_flush, t, block_min);
        if (r.status != kInfOverflow && r.cut != kInfOverflow) {
            out.resize(base + (size_t)r.out_len);
            return r;
        }
        cap *= 2;
    }
}

int gunzip_serial(const uint8_t* gz, size_t n, std::vector<uint8_t>& out)
{
    size_t at = 0;
    if (n == 0) return SNAPHASH_EFORMAT; // (gzip.NewReader: io.EOF before the first header)
    while (at < n) {
        size_t h = 0;
        if (gzip_header(gz + at, n - at, &h)) return SNAPHASH_EFORMAT;
        const size_t m0 = out.size();
        const InflateRun r = inflate_host_append(gz + at + h, n - at - h, 0, out, m0, false);
        if (r.status != kInfFinal) return SNAPHASH_EFORMAT;
        const uint32_t crc = crc32_update(0, out.data() + m0, out.size() - m0);
        size_t next = 0;
        if (gzip_trailer(gz + at + h, n - at - h, r.end_bit, crc, out.size() - m0, &next)) return SNAPHASH_EFORMAT;
        at += h + next;
    }
    return 0;
}

std::vector<uint64_t> flush_candidates(const uint8_t* in, size_t n)
{
    // a possible stored block: LEN and NLEN = ~LEN at j..j+3; the next block would start at j + 4 + LEN.  An empty one
    // is the flush marker and always counts; a stored chunk only where the byte in front can hold its header bits with
    // zero padding (< 32: what zlib, Go and the producer write), which keeps the false ones rare
    std::vector<uint64_t> c;
    for (size_t j = 0; j + 4 <= n; ++j) {
        const uint32_t len = in[j] | (uint32_t)in[j + 1] << 8, nlen = in[j + 2] | (uint32_t)in[j + 3] << 8;
        if (len != (~nlen & 0xffffu)) continue;
        if (len != 0 && (j == 0 || in[j - 1] >= 32)) continue;
        if (j + 4 + len <= n) c.push_back(j + 4 + len);
    }
    std::sort(c.begin(), c.end());
    c.erase(std::unique(c.begin(), c.end()), c.end());
    return c;
}

bool fill_holes_host(const uint16_t* seg, size_t len, uint8_t* out_base, size_t avail)
{
    for (size_t p = 0; p < len; ++p) {
        const uint32_t v = seg[p];
        if (v < kInfHole) { out_base[p] = (uint8_t)v; continue; }
        const size_t w = v - kInfHole;
        if (w > avail) return false;
        out_base[p] = *(out_base - w); // (a byte of an earlier segment: already final)
    }
    return true;
}

int inflate_segments_host(const uint8_t* in, size_t n, const uint64_t* starts, size_t nstarts, std::vector<uint8_t>& out,
                          unsigned threads, uint64_t* end_bit)
{
    if (nstarts == 0 || starts[0] != 0) return SNAPHASH_EFORMAT;
    std::vector<std::vector<uint16_t>> seg(nstarts);
    std::vector<InflateRun> run(nstarts);
    std::atomic<size_t> next{0};
    auto work = [&]() {
        InflateTables t;
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= nstarts) return;
            const uint64_t lim = i + 1 < nstarts ? starts[i + 1] : n;
            // a stretch may hold several segments (stored blocks end them too): run on until the next start is reached
            size_t cap = std::max<size_t>((size_t)(lim - starts[i]) * 4, 1u << 16), o = 0;
            uint64_t bit = starts[i] * 8;
            seg[i].resize(cap);
            for (;;) {
                InflateRun r = inflate_run<uint16_t>(in, n, bit, seg[i].data() + o, o, cap - o, true, true, t);
                if (r.status == kInfOverflow) { cap *= 2; seg[i].resize(cap); continue; }
                o += (size_t)r.out_len;
                bit = r.end_bit;
                run[i] = r;
                if (r.status != kInfFlush || (i + 1 < nstarts && bit >= starts[i + 1] * 8)) break;
            }
            seg[i].resize(o);
        }
    };
    threads = (unsigned)std::max<size_t>(1, std::min<size_t>(threads, nstarts));
    std::vector<std::thread> th;
    for (unsigned k = 1; k < threads; ++k) th.emplace_back(work);
    work();
    for (auto& x : th) x.join();
    const size_t m0 = out.size();
    for (size_t i = 0; i < nstarts; ++i) {
        const bool last = i + 1 == nstarts;
        if (last ? run[i].status != kInfFinal : (run[i].status != kInfFlush || run[i].end_bit != starts[i + 1] * 8))
            return SNAPHASH_EFORMAT;
        const size_t base = out.size();
        out.resize(base + seg[i].size());
        if (!fill_holes_host(seg[i].data(), seg[i].size(), out.data() + base, base - m0)) return SNAPHASH_EFORMAT;
    }
    *end_bit = run[nstarts - 1].end_bit;
    return 0;
}

} // namespace snaphash
