// asan_deflate_check.cpp -- the self-check's walker (snappy_amd/csrc/deflate_check_core.h) as a program of its own for
// -fsanitize=address,undefined (tests/test_snapbuild_host.py builds and runs it; nothing here is loaded into python).
// Argument: a file of streams, each four little-endian u64 (n_in, n_z, nchunks, last_is_final), the staged bytes, the
// compressed bytes and nchunks + 1 u64 offsets.  Every stream goes through deflate_check_entry chunk by chunk with both
// buffers on the heap at exactly their size, so that a read one byte outside either is reported; then once more with every
// stretch cut short by one byte and with the table's entries moved by one, which must end as cleanly.  Prints the counts.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../snappy_amd/csrc/deflate_check_core.h"

using namespace snaphash;

static bool get64(FILE* f, uint64_t* v)
{
    uint8_t b[8];
    if (fread(b, 1, 8, f) != 8) return false;
    *v = 0;
    for (int i = 7; i >= 0; --i) *v = *v << 8 | b[i];
    return true;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("open\n"); return 2; }
    uint64_t streams = 0, walks = 0, accepted = 0;
    InflateTables* t = new InflateTables;
    for (;;) {
        uint64_t n_in, n_z, nch, final;
        if (!get64(f, &n_in)) break;
        if (!get64(f, &n_z) || !get64(f, &nch) || !get64(f, &final)) { printf("header\n"); return 2; }
        if (n_in > (1u << 26) || n_z > (1u << 26) || nch == 0 || nch > 4096) { printf("length\n"); return 2; }
        uint8_t* in = (uint8_t*)malloc(n_in ? n_in : 1); // (malloc(0) may return null)
        uint8_t* z = (uint8_t*)malloc(n_z ? n_z : 1);
        std::vector<uint64_t> off(nch + 1);
        if (fread(in, 1, n_in, f) != n_in || fread(z, 1, n_z, f) != n_z) { printf("short read\n"); return 2; }
        for (uint64_t& o : off)
            if (!get64(f, &o)) { printf("short read\n"); return 2; }
        ++streams;
        for (int pass = 0; pass < 4; ++pass) {
            std::vector<uint64_t> o2 = off;
            uint64_t total = n_z;
            if (pass == 1 && total) --total;                        // the buffer one byte shorter than the table says
            if (pass == 2) for (size_t k = 1; k < o2.size(); ++k) o2[k] += 1; // every stretch one byte late
            if (pass == 3) for (size_t k = 1; k + 1 < o2.size(); ++k) if (o2[k]) o2[k] -= 1;
            uint8_t* zz = (uint8_t*)malloc(total ? total : 1);
            for (uint64_t i = 0; i < total; ++i) zz[i] = z[i];
            for (uint32_t c = 0; c < nch; ++c) {
                const DfCheckVerdict v = deflate_check_entry(in, n_in, zz, total, o2.data(), nullptr, c, final && c + 1 == nch, *t);
                ++walks;
                accepted += v.status == kDfCheckOk;
            }
            free(zz);
        }
        free(in);
        free(z);
    }
    fclose(f);
    delete t;
    printf("%llu streams, %llu walks, %llu accepted\n", (unsigned long long)streams, (unsigned long long)walks, (unsigned long long)accepted);
    return 0;
}
