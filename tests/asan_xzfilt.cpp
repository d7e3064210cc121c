// asan_xzfilt.cpp -- the PowerPC, IA64, SPARC and Delta filters (snappy_amd/csrc/bcj_core.h, delta_core.h) as a program of
// its own for -fsanitize=address,undefined (tests/test_xzfilt_host.py builds and runs it; nothing here is loaded into
// python).  Arguments: triples of (input file, filter id, parameter: a BCJ filter's start_offset, Delta's distance).  Each
// input is read into a heap buffer of exactly its size; in both directions the Block is filtered on one thread and by the
// kernels' pieces (the word filters stretch by stretch at 256 and 16 bytes; Delta tile by tile at 65 536, 64 and 8 bytes; in
// both orders), every copy on the heap at exactly its size; the pieces must give the serial bytes, and decoding what was
// encoded the input.  "ok" a triple, exit 0 when all are.
#include <stdio.h>

#include "xzfilt_host_harness.cpp"

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
    bool operator==(const Exact& o) const { return n == o.n && (n == 0 || memcmp(p, o.p, n) == 0); }
};

bool pieces_equal(uint32_t id, uint32_t param, bool encode, const Exact& in, const Exact& want)
{
    bool ok = true;
    for (int order = 0; order < 2; ++order) {
        if (id == kXzDelta) {
            for (uint64_t tile : {65536ull, 64ull, 8ull}) {
                if (tile < 65536 && in.n > 70000 && order) continue; // (the long inputs at the small tiles: one order)
                Exact b(in.p, in.n);
                xf_delta_tiles(encode, b.p, b.n, param, tile, kDeltaLanes, order);
                ok = ok && b == want;
            }
        } else {
            for (uint32_t stretch : {256u, 16u}) {
                Exact b(in.p, in.n);
                xf_cut(id, encode, b.p, b.n, param, stretch, order);
                ok = ok && b == want;
            }
        }
    }
    return ok;
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
        const uint32_t id = (uint32_t)strtoul(argv[i + 1], nullptr, 10), param = (uint32_t)strtoul(argv[i + 2], nullptr, 10);
        const uint32_t dist = id == kXzDelta ? param : 0, start = id == kXzDelta ? 0 : param;
        Exact enc(in.p, n);
        bool ok = xf_block(id, dist, 1, enc.p, n, start) == 0;
        Exact back(enc.p, n);
        ok = ok && xf_block(id, dist, 0, back.p, n, start) == 0 && back == in;
        Exact dec(in.p, n);
        ok = ok && xf_block(id, dist, 0, dec.p, n, start) == 0;
        ok = ok && pieces_equal(id, param, true, in, enc) && pieces_equal(id, param, false, in, dec);
        printf(ok ? "ok\n" : "FAILED\n");
        bad += !ok;
    }
    return bad ? 1 : 0;
}
