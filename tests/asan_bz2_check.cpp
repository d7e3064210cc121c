// asan_bz2_check.cpp -- the .bz2 self-check's host model (snappy_amd/csrc/bz2_check_core.h) as a program of its own for
// -fsanitize=address,undefined (tests/test_bz2_check_host.py builds and runs it; nothing here is loaded into python).
// Argument: a file of cases, each four little-endian u64 (n_z, n_in, blocks, level), the compressed bytes, the staged bytes
// and five tables of `blocks` u64 each (z_beg, z_end, in_off, in_len, crc).  Every case goes through bz2_check_block block by
// block with both buffers on the heap at exactly their size, so that a read one byte outside either is reported; then again
// with the compressed buffer one byte shorter than the tables say, with the staged buffer one byte shorter, and with the
// tables' entries moved by one either way, which must end as cleanly.  Prints the counts; the first pass's verdicts go to the
// file named by the second argument, two u32 a block, for the test to hold against the harness's.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/snaphash.h"
#include "../snappy_amd/csrc/bzip2_host.cpp"
#include "../snappy_amd/csrc/bz2_check_core.h"

using namespace snaphash;

static bool get64(FILE* f, uint64_t* v)
{
    uint8_t b[8];
    if (fread(b, 1, 8, f) != 8) return false;
    *v = 0;
    for (int i = 7; i >= 0; --i) *v = *v << 8 | b[i];
    return true;
}

static uint8_t* heap_copy(const uint8_t* p, uint64_t n)
{
    uint8_t* q = (uint8_t*)malloc(n ? n : 1); // (malloc(0) may return null)
    if (n) memcpy(q, p, n);
    return q;
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* vf = fopen(argv[2], "wb");
    if (!f || !vf) { printf("open\n"); return 2; }
    uint64_t cases = 0, checks = 0, accepted = 0;
    BzScratch s;
    for (;;) {
        uint64_t n_z, n_in, nb, level;
        if (!get64(f, &n_z)) break;
        if (!get64(f, &n_in) || !get64(f, &nb) || !get64(f, &level)) { printf("header\n"); return 2; }
        if (n_z > (1u << 26) || n_in > (1u << 26) || nb == 0 || nb > 4096 || level < 1 || level > 9) { printf("length\n"); return 2; }
        std::vector<uint8_t> z(n_z), in(n_in);
        std::vector<uint64_t> tab[5];
        if (fread(z.data(), 1, n_z, f) != n_z || fread(in.data(), 1, n_in, f) != n_in) { printf("short read\n"); return 2; }
        for (auto& t : tab) {
            t.resize(nb);
            for (uint64_t& o : t)
                if (!get64(f, &o)) { printf("short read\n"); return 2; }
        }
        ++cases;
        for (int pass = 0; pass < 7; ++pass) {
            std::vector<uint64_t> zb = tab[0], ze = tab[1], io = tab[2], il = tab[3];
            uint64_t zn = n_z, inn = n_in;
            if (pass == 1 && zn) --zn;   // the compressed buffer one byte shorter than the tables say
            if (pass == 2 && inn) --inn; // the staged buffer one byte shorter
            if (pass == 3) for (size_t k = 0; k < nb; ++k) { zb[k] += 1; ze[k] += 1; } // every stretch one bit late
            if (pass == 4) for (size_t k = 0; k < nb; ++k) { if (zb[k]) zb[k] -= 1; if (ze[k]) ze[k] -= 1; }
            if (pass == 5) for (size_t k = 0; k < nb; ++k) io[k] += 1;                  // every piece one byte late
            if (pass == 6) for (size_t k = 0; k < nb; ++k) il[k] += 1;                  // every piece one byte longer
            uint8_t* hz = heap_copy(z.data(), zn);
            uint8_t* hin = heap_copy(in.data(), inn);
            for (size_t k = 0; k < nb; ++k) {
                const Bz2CheckJob j = {zb[k], ze[k], io[k], il[k], (uint32_t)tab[4][k], 0};
                const Bz2Verdict v = bz2_check_block(hz, zn, hin, inn, j, (uint32_t)level, s);
                ++checks;
                accepted += v.status == kBz2CheckOk;
                if (pass == 0 && fwrite(&v, sizeof v, 1, vf) != 1) { printf("write\n"); return 2; }
            }
            free(hz);
            free(hin);
        }
    }
    fclose(f);
    if (fclose(vf) != 0) { printf("write\n"); return 2; }
    printf("%llu cases, %llu checks, %llu accepted\n", (unsigned long long)cases, (unsigned long long)checks, (unsigned long long)accepted);
    return 0;
}
