// asan_bcj.cpp -- the BCJ filters (snappy_amd/csrc/bcj_core.h) as a program of its own for -fsanitize=address,undefined
// (tests/test_bcj_host.py builds and runs it; nothing here is loaded into python).  Arguments: triples of (input file,
// filter id, start_offset).  Each input is read into a heap buffer of exactly its size; in both directions the Block is
// filtered on one thread and by the kernels' cut (stretches of 256 and of 8 bytes, in both orders), every copy on the heap
// at exactly its size, the points table at exactly its count; the cuts must give the serial bytes, and decoding what was
// encoded the input.  "ok" a triple, exit 0 when all are.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../snappy_amd/csrc/bcj_core.h"

using namespace snaphash;

namespace {

struct Exact { // n bytes on the heap, no more (malloc(0) may be null: one byte that is never passed on)
    uint8_t* p;
    size_t n;
    explicit Exact(const uint8_t* src, size_t n_) : p((uint8_t*)malloc(n_ ? n_ : 1)), n(n_)
    {
        if (n) memcpy(p, src, n);
    }
    ~Exact() { free(p); }
    Exact(const Exact&) = delete;
    Exact& operator=(const Exact&) = delete;
};

bool cut_equals(uint32_t filter, bool encode, const Exact& in, const Exact& want, uint32_t start, uint32_t stretch, int order)
{
    Exact b(in.p, in.n);
    const uint64_t nk = (in.n + stretch - 1) / stretch;
    uint32_t* points = (uint32_t*)malloc(nk ? nk * 4 : 1);
    if (filter == kBcjX86)
        for (uint64_t k = 0; k < nk; ++k) points[k] = bcj_x86_stretch_point(b.p, b.n, k, stretch);
    for (uint64_t i = 0; i < nk; ++i) bcj_stretch_apply(filter, encode, b.p, b.n, order ? nk - 1 - i : i, nk, stretch, points, start);
    free(points);
    return in.n == 0 || memcmp(b.p, want.p, in.n) == 0;
}

} // namespace

int main(int argc, char** argv)
{
    int bad = 0;
    for (int i = 1; i + 2 < argc; i += 3) {
        FILE* f = fopen(argv[i], "rb");
        if (!f) { printf("open\n"); return 2; }
        std::vector<uint8_t> big(4u << 20);
        const size_t n = fread(big.data(), 1, big.size(), f);
        fclose(f);
        const Exact in(big.data(), n);
        std::vector<uint8_t>().swap(big);
        const uint32_t filter = (uint32_t)strtoul(argv[i + 1], nullptr, 10), start = (uint32_t)strtoul(argv[i + 2], nullptr, 10);
        bool ok = bcj_filter_valid(filter) && (start & (bcj_alignment(filter) - 1)) == 0;
        Exact enc(in.p, n);
        bcj_block(filter, true, enc.p, n, start);
        Exact back(enc.p, n);
        bcj_block(filter, false, back.p, n, start);
        ok = ok && (n == 0 || memcmp(back.p, in.p, n) == 0);
        Exact dec(in.p, n);
        bcj_block(filter, false, dec.p, n, start);
        for (uint32_t stretch : {256u, 8u})
            for (int order = 0; order < 2; ++order) {
                ok = ok && cut_equals(filter, true, in, enc, start, stretch, order);
                ok = ok && cut_equals(filter, false, in, dec, start, stretch, order);
            }
        printf(ok ? "ok\n" : "FAILED\n");
        bad += !ok;
    }
    return bad ? 1 : 0;
}
