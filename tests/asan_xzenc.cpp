// asan_xzenc.cpp -- the .xz writer's host model (snappy_amd/csrc/xz_enc_core.h) and the host decoder over what it wrote,
// as a program of its own for -fsanitize=address,undefined (tests/test_xzenc_host.py builds and runs it; nothing here is
// loaded into python).  Arguments: pairs of (input file, block size).  Each input is read into a heap buffer of exactly
// its size, encoded, decoded again and compared: "ok" a pair, exit 0 when all are.
#include <stdio.h>
#include <stdlib.h>

#include "../snappy_amd/csrc/xz_host.cpp"
#include "../snappy_amd/csrc/xz_enc_core.h"

using namespace snaphash;

int main(int argc, char** argv)
{
    int bad = 0;
    for (int i = 1; i + 1 < argc; i += 2) {
        FILE* f = fopen(argv[i], "rb");
        if (!f) { printf("open\n"); return 2; }
        std::vector<uint8_t> big(8u << 20);
        const size_t n = fread(big.data(), 1, big.size(), f);
        fclose(f);
        std::vector<uint8_t> exact(big.begin(), big.begin() + (long)n); // (no byte behind the input may be read)
        std::vector<uint8_t>().swap(big);
        const uint64_t bs = strtoull(argv[i + 1], nullptr, 10);
        std::vector<uint8_t> z, back;
        NoEncOps ops;
        XzEncInfo info;
        std::string why;
        bool ok = xzenc_host(exact.data(), exact.size(), bs, z, ops, [](const uint8_t* p, uint64_t len) { return xz_crc64(p, len); }, &info);
        std::vector<uint8_t> zexact(z);
        ok = ok && xz_decode_host(zexact.data(), zexact.size(), back, 2, nullptr, why) == 0 && back == exact;
        ok = ok && info.chunks == (exact.size() + kXzEncChunk - 1) / kXzEncChunk;
        printf(ok ? "ok\n" : "FAILED\n");
        bad += !ok;
    }
    // a refused block size touches nothing
    std::vector<uint8_t> z;
    NoEncOps ops;
    const uint8_t one = 1;
    if (xzenc_host(&one, 1, (4u << 20) + 65536, z, ops, [](const uint8_t*, uint64_t) { return (uint64_t)0; })) ++bad;
    return bad ? 1 : 0;
}
