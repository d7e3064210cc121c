// asan_tarread.cpp -- the tar reader (snappy_amd/csrc/tar_core.h) as a program of its own for
// -fsanitize=address,undefined (tests/test_tar_host.py builds and runs it; nothing here is loaded into python).  Argument:
// a file of archives, each a little-endian u64 length and that many bytes.  Every archive goes through tar_read from a
// heap buffer of exactly its size; then every 512-byte block of it that holds a non-zero byte is taken for a header and
// each of its numeric fields set to the sweep's four values (tests/tar_sweep.h), the checksum as it was and put right.
// The extent invariant is checked on every result.  Prints the counts; exit 0 when nothing broke it.
#include <stdio.h>
#include <stdlib.h>

#include "tar_sweep.h"

using namespace tarsweep;

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("open\n"); return 2; }
    uint64_t archives = 0, runs = 0;
    int bad = 0;
    for (;;) {
        uint8_t l8[8];
        if (fread(l8, 1, 8, f) != 8) break;
        uint64_t n = 0;
        for (int i = 7; i >= 0; --i) n = n << 8 | l8[i];
        if (n > (1u << 24)) { printf("length\n"); return 2; }
        Sweep sw;
        sw.buf.resize((size_t)n);
        if (fread(sw.buf.data(), 1, (size_t)n, f) != n) { printf("short read\n"); return 2; }
        ++archives;
        bool ok = sw.run();
        for (uint64_t h = 0; ok && n - h >= 512; h += 512) {
            bool any = false;
            for (int i = 0; i < 512 && !any; ++i) any = sw.buf[h + i] != 0;
            if (any) ok = sw.fields(h);
        }
        runs += sw.runs;
        if (!ok) { printf("archive %llu: an entry leaves the stream (mutation at byte %llu)\n", (unsigned long long)archives - 1, (unsigned long long)sw.broken_at); ++bad; }
    }
    fclose(f);
    printf("%llu archives, %llu runs of tar_read, %d broke the invariant\n", (unsigned long long)archives, (unsigned long long)runs, bad);
    return bad ? 1 : 0;
}
