// Host harness of the install side's decoder (snappy_amd/csrc/inflate_core.h + inflate_host.cpp): the one-core gunzip,
// the raw decode from a start bit, and the segmented decode with holes, for tests/test_inflate_host.py.  Built with
// -DIH_MAIN it is a program that decodes mutated copies of a stream (run under ASan + UBSan by the same test).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "../include/snaphash.h"
#include "../snappy_amd/csrc/inflate_host.cpp"
#include "../snappy_amd/csrc/tarpack.cpp"
#include "../snappy_amd/csrc/walk.cpp"
#include "../snappy_amd/csrc/hostfill.cpp" // walk.cpp sizes its thread pools with usable_cpus()

using namespace snaphash;

static void* give(const std::vector<uint8_t>& v, size_t* len)
{
    void* p = malloc(v.size() + 1);
    if (!v.empty()) memcpy(p, v.data(), v.size());
    *len = v.size();
    return p;
}

extern "C" {

void* ih_gunzip(const uint8_t* gz, size_t n, size_t* len, int* rc)
{
    std::vector<uint8_t> out;
    *rc = gunzip_serial(gz, n, out);
    return give(out, len);
}

// a raw DEFLATE stream from bit 0 to its final block; the status of inflate_run, *end_bit where it stopped
void* ih_inflate_raw(const uint8_t* in, size_t n, size_t* len, int* status, uint64_t* end_bit)
{
    std::vector<uint8_t> out;
    const InflateRun r = inflate_host_append(in, n, 0, out, 0, false);
    *status = r.status;
    *end_bit = r.end_bit;
    return give(out, len);
}

// one segment in hole mode: the uint16 symbols (kInfHole + w for a hole), the status, the end bit and hole_end
void* ih_segment(const uint8_t* in, size_t n, uint64_t start_bit, size_t cap, size_t* len, int* status, uint64_t* end_bit, uint32_t* hole_end)
{
    InflateTables t;
    std::vector<uint16_t> seg(cap + 1);
    const InflateRun r = inflate_run<uint16_t>(in, n, start_bit, seg.data(), 0, cap, true, true, t);
    *status = r.status;
    *end_bit = r.end_bit;
    *hole_end = r.hole_end;
    *len = (size_t)r.out_len;
    void* p = malloc(2 * (size_t)r.out_len + 2);
    memcpy(p, seg.data(), 2 * (size_t)r.out_len);
    return p;
}

void* ih_segments(const uint8_t* in, size_t n, const uint64_t* starts, size_t ns, unsigned threads, size_t* len, int* rc)
{
    std::vector<uint8_t> out;
    uint64_t end_bit = 0;
    *rc = inflate_segments_host(in, n, starts, ns, out, threads, &end_bit);
    return give(out, len);
}

size_t ih_candidates(const uint8_t* in, size_t n, uint64_t* out, size_t cap)
{
    const std::vector<uint64_t> c = flush_candidates(in, n);
    for (size_t i = 0; i < c.size() && i < cap; ++i) out[i] = c[i];
    return c.size();
}

void ih_free(void* p) { free(p); }

} // extern "C"

#ifdef IH_MAIN
// ih_fuzz <gz file> <count> <seed>: decodes `count` mutated or truncated copies of the stream, serially and (raw
// DEFLATE after the 10-byte header) segment by segment from every flush candidate; any out-of-bounds access or UB is the
// sanitizers' to report.  Prints how many decodes returned 0.
int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> gz;
    uint8_t buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) gz.insert(gz.end(), buf, buf + k);
    fclose(f);
    const long count = atol(argv[2]);
    std::mt19937_64 rng((uint64_t)atoll(argv[3]));
    long ok = 0;
    for (long it = 0; it < count; ++it) {
        std::vector<uint8_t> m = gz;
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
        std::vector<uint8_t> out;
        if (gunzip_serial(m.data(), m.size(), out) == 0) ++ok;
        if (m.size() > 10) {
            const uint8_t* raw = m.data() + 10;
            const size_t rn = m.size() - 10;
            std::vector<uint64_t> starts{0};
            for (uint64_t c : flush_candidates(raw, rn)) starts.push_back(c);
            std::vector<uint8_t> o2;
            uint64_t end_bit = 0;
            (void)inflate_segments_host(raw, rn, starts.data(), starts.size(), o2, 1, &end_bit);
        }
    }
    printf("%ld\n", ok);
    return 0;
}
#endif
