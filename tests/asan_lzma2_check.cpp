// asan_lzma2_check.cpp -- the .xz self-check's walker (snappy_amd/csrc/lzma2_check_core.h) as a program of its own for
// -fsanitize=address,undefined (tests/test_lzma2_check_host.py builds and runs it; nothing here is loaded into python).
// Argument: a file of streams, each four little-endian u64 (n_in, n_z, nchunks, block size), the staged bytes, the
// compressed bytes and the two tables of nchunks u64 each (z_beg, z_end).  Every stream goes through lzma2_check_chunk chunk
// by chunk with both buffers on the heap at exactly their size, so that a read one byte outside either is reported; then
// again with the compressed buffer one byte shorter than the tables say, with the staged buffer one byte shorter, and with
// the tables' entries moved by one either way, which must end as cleanly.  Prints the counts; the first pass's verdicts go
// to the file named by the second argument, two u32 a chunk, for the test to hold against the harness's.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../snappy_amd/csrc/lzma2_check_core.h"

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
    uint64_t streams = 0, walks = 0, accepted = 0;
    std::vector<uint16_t> probs(kLzCheckProbs);
    for (;;) {
        uint64_t n_in, n_z, nch, bs;
        if (!get64(f, &n_in)) break;
        if (!get64(f, &n_z) || !get64(f, &nch) || !get64(f, &bs)) { printf("header\n"); return 2; }
        if (n_in == 0 || n_in > (1u << 26) || n_z > (1u << 26) || nch != (n_in + kLzCheckChunk - 1) / kLzCheckChunk || bs == 0 || bs % kLzCheckChunk)
        {
            printf("length\n");
            return 2;
        }
        std::vector<uint8_t> in(n_in), z(n_z);
        std::vector<uint64_t> beg(nch), end(nch);
        if (fread(in.data(), 1, n_in, f) != n_in || fread(z.data(), 1, n_z, f) != n_z) { printf("short read\n"); return 2; }
        for (uint64_t& o : beg)
            if (!get64(f, &o)) { printf("short read\n"); return 2; }
        for (uint64_t& o : end)
            if (!get64(f, &o)) { printf("short read\n"); return 2; }
        ++streams;
        for (int pass = 0; pass < 6; ++pass) {
            std::vector<uint64_t> b2 = beg, e2 = end;
            uint64_t zn = n_z, inn = n_in;
            if (pass == 1 && zn) --zn;   // the compressed buffer one byte shorter than the tables say
            if (pass == 2) --inn;        // the staged buffer one byte shorter: the last chunk loses a byte, or goes
            if (pass == 3) for (size_t k = 0; k < nch; ++k) { b2[k] += 1; e2[k] += 1; } // every stretch one byte late
            if (pass == 4) for (size_t k = 0; k < nch; ++k) { if (b2[k]) b2[k] -= 1; if (e2[k]) e2[k] -= 1; }
            if (pass == 5) for (size_t k = 0; k < nch; ++k) e2[k] += 1;               // every stretch one byte longer
            if (inn == 0) continue;
            uint8_t* hin = heap_copy(in.data(), inn);
            uint8_t* hz = heap_copy(z.data(), zn);
            const uint64_t n2 = (inn + kLzCheckChunk - 1) / kLzCheckChunk;
            for (uint32_t c = 0; c < n2; ++c) {
                const Lzma2Verdict v = lzma2_check_chunk(hin, inn, bs, hz, zn, b2[c], e2[c], c, probs.data());
                ++walks;
                accepted += v.status == kLzCheckOk;
                if (pass == 0 && fwrite(&v, sizeof v, 1, vf) != 1) { printf("write\n"); return 2; }
            }
            free(hin);
            free(hz);
        }
    }
    fclose(f);
    if (fclose(vf) != 0) { printf("write\n"); return 2; }
    printf("%llu streams, %llu walks, %llu accepted\n", (unsigned long long)streams, (unsigned long long)walks, (unsigned long long)accepted);
    return 0;
}
