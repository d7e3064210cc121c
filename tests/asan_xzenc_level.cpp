// asan_xzenc_level.cpp -- the .xz writer's host model at level 1 (snappy_amd/csrc/xz_enc_core.h) and the
// host decoder over what it wrote, as a program of its own for -fsanitize=address,undefined (tests/test_xzenc_level_host.py
// builds and runs it; nothing here is loaded into python).  Arguments: pairs of (input file, block size).  Each input is
// read into a heap buffer of exactly its size, encoded at level 1 with the lanes in ascending and in descending order,
// decoded again and compared: "ok" a pair, exit 0 when all are.
#include <stdio.h>
#include <stdlib.h>

#include "../snappy_amd/csrc/xz_host.cpp"
#include "../snappy_amd/csrc/xz_enc_core.h"

using namespace snaphash;

int main(int argc, char** argv)
{
    int bad = 0;
    const auto field = [](const uint8_t* p, uint64_t len, uint8_t* f) { xzenc_le64(f, xz_crc64(p, len)); };
    for (int i = 1; i + 1 < argc; i += 2) {
        FILE* f = fopen(argv[i], "rb");
        if (!f) { printf("open\n"); return 2; }
        std::vector<uint8_t> big(8u << 20);
        const size_t n = fread(big.data(), 1, big.size(), f);
        fclose(f);
        std::vector<uint8_t> exact(big.begin(), big.begin() + (long)n); // (no byte behind the input may be read)
        std::vector<uint8_t>().swap(big);
        const uint64_t bs = strtoull(argv[i + 1], nullptr, 10);
        std::vector<uint8_t> z, zd, back;
        NoEncOps ops;
        XzEncInfo info;
        std::string why;
        bool ok = xzenc_host(exact.data(), exact.size(), bs, (uint32_t)kXzCheckCrc64, z, ops, field, &info, 0, 1, false);
        ok = ok && xzenc_host(exact.data(), exact.size(), bs, (uint32_t)kXzCheckCrc64, zd, ops, field, nullptr, 0, 1, true) && zd == z;
        std::vector<uint8_t> zexact(z);
        ok = ok && xz_decode_host(zexact.data(), zexact.size(), back, 2, nullptr, why) == 0 && back == exact;
        ok = ok && info.chunks == (exact.size() + kXzEncChunk - 1) / kXzEncChunk;
        printf(ok ? "ok\n" : "FAILED\n");
        bad += !ok;
    }
    // a level that does not exist touches nothing
    std::vector<uint8_t> z;
    NoEncOps ops;
    const uint8_t one = 1;
    if (xzenc_host(&one, 1, 65536, (uint32_t)kXzCheckCrc64, z, ops, field, nullptr, 0, 2) || !z.empty()) ++bad;
    return bad ? 1 : 0;
}
