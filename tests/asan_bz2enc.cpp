// asan_bz2enc.cpp -- the .bz2 writer's host model (snappy_amd/csrc/bzip2_enc_core.h) and bzip2_core.h's decoder over what
// it wrote, as a program of its own for -fsanitize=address,undefined (tests/test_bz2enc_host.py builds and runs it; nothing
// here is loaded into python).  Arguments: a count of random inputs, a seed, then pairs of (input file, level).  Each
// input is read into a heap buffer of exactly its size, encoded, decoded block by block with bz_block_symbols / bz_ibwt /
// bz_rle1 and compared: "ok" an input, exit 0 when all are.
#include <stdio.h>
#include <stdlib.h>

#include "../snappy_amd/csrc/bzip2_enc_core.h"

using namespace snaphash;

static bool round_trip(const std::vector<uint8_t>& exact, uint32_t level)
{
    std::vector<BzEncBlockInfo> infos;
    const std::vector<uint8_t> z0 = bzenc_stream_host(exact.data(), exact.size(), level, &infos);
    std::vector<uint8_t> z(z0); // (exactly its size)
    if (z.size() < 14 || z[0] != 'B' || z[1] != 'Z' || z[2] != 'h' || z[3] != '0' + level) return false;
    const uint32_t P = bzenc_piece(level);
    if (infos.size() != (exact.size() + P - 1) / P) return false;
    std::vector<uint8_t> back, bwt(kBzMaxBlock), plain(kBzMaxBlock);
    std::vector<uint32_t> tt(kBzMaxBlock);
    std::vector<BzTables> t(1);
    uint32_t crc_tab[256];
    bz_crc_table(crc_tab);
    uint64_t bit = 32;
    uint32_t fold = 0;
    for (size_t k = 0; k < infos.size(); ++k) {
        uint32_t counts[256];
        const BzBlockRes r = bz_block_symbols(z.data(), z.size(), bit, bwt.data(), kBzMaxBlock, counts, t[0]);
        if (r.status != kBzOk || r.n != infos[k].rle_n || r.orig_ptr != infos[k].orig_ptr || r.end_bit - bit != infos[k].bits) return false;
        bz_ibwt(bwt.data(), r.n, counts, r.orig_ptr, tt.data(), plain.data());
        BzRle1 st;
        const uint64_t at = back.size();
        const uint64_t len = bz_rle1(st, plain.data(), r.n, nullptr, 0);
        back.resize(at + len);
        BzRle1 st2;
        if (bz_rle1(st2, plain.data(), r.n, back.data() + at, len) != len) return false;
        if (~bz_crc_update(crc_tab, ~0u, back.data() + at, len) != r.crc) return false;
        fold = bz_crc_combine(fold, r.crc);
        bit = r.end_bit;
    }
    if (bz_bits48(z.data(), z.size(), bit) != kBzEosMagic) return false;
    BzBits b;
    bb_start(b, z.data(), z.size(), bit + 48);
    if (bb_take(b, 32) != fold) return false;
    return back == exact && (bit + 80 + 7) / 8 == z.size();
}

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const long nrandom = strtol(argv[1], nullptr, 10);
    uint64_t seed = strtoull(argv[2], nullptr, 10) * 2654435761u + 1;
    auto next = [&seed]() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return seed; };
    int bad = 0;
    for (int i = 3; i + 1 < argc; i += 2) {
        FILE* f = fopen(argv[i], "rb");
        if (!f) { printf("open\n"); return 2; }
        std::vector<uint8_t> big(8u << 20);
        const size_t n = fread(big.data(), 1, big.size(), f);
        fclose(f);
        std::vector<uint8_t> exact(big.begin(), big.begin() + (long)n); // (no byte behind the input may be read)
        std::vector<uint8_t>().swap(big);
        const bool ok = round_trip(exact, (uint32_t)strtoul(argv[i + 1], nullptr, 10));
        printf(ok ? "ok\n" : "FAILED\n");
        bad += !ok;
    }
    // random inputs of random length and level: alphabets of 1 to 256 values, with and without runs
    long good = 0;
    for (long k = 0; k < nrandom; ++k) {
        const uint64_t shape = next();
        size_t n = (size_t)(next() % ((shape & 15) == 0 ? 200u * 1024 + 1 : 3000));
        const uint32_t level = 1 + (uint32_t)(next() % 9), alpha = 1 + (uint32_t)(next() % 256), runs = (uint32_t)(shape >> 8 & 3);
        std::vector<uint8_t> exact(n);
        for (size_t i = 0; i < n;) {
            const uint8_t v = (uint8_t)(next() % alpha);
            size_t len = runs == 0 ? 1 : 1 + (size_t)(next() % (runs == 1 ? 6 : 600));
            for (; len && i < n; --len) exact[i++] = v;
        }
        if (round_trip(exact, level)) ++good;
        else { printf("FAILED random %ld (n %zu level %u alpha %u runs %u)\n", k, n, level, alpha, runs); ++bad; }
    }
    printf("random %ld\n", good);
    return bad ? 1 : 0;
}
