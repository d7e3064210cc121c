// snapbuild_host_harness.cpp -- the build side's host-only parts for tests/test_snapbuild_host.py (built into a shared object
// with g++ and loaded with ctypes): the ar writer and reader of snappy_amd/csrc/snap_core.h, and the self-check's walker
// (snappy_amd/csrc/deflate_check_core.h), which the GPU kernel compiles from the same header.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../snappy_amd/csrc/deflate_check_core.h"
#include "../snappy_amd/csrc/snap_core.h"

using namespace snaphash;

extern "C" {

// n members: names NUL-terminated one after another, sizes[i] bytes each out of data one after another.
// -> ar_write's code; the container in out (at most cap bytes), its length in *out_len.
int sb_ar_write(const char* names, const uint64_t* sizes, size_t n, const uint8_t* data, int64_t mtime, uint32_t mode, uint8_t* out, size_t cap,
                uint64_t* out_len)
{
    std::vector<ArInput> mem(n);
    for (size_t i = 0; i < n; ++i) {
        mem[i].name = names;
        names += mem[i].name.size() + 1;
        mem[i].data = data;
        mem[i].size = sizes[i];
        data += sizes[i];
    }
    std::vector<uint8_t> v;
    const int rc = ar_write(mem, mtime, mode, v);
    *out_len = v.size();
    if (v.size() > cap) return 99;
    if (!v.empty()) memcpy(out, v.data(), v.size());
    return rc;
}

// ar_parse's code; per member a line "hexname\toffset\tsize" in text
int sb_ar_parse(const uint8_t* p, uint64_t n, char* text, size_t cap)
{
    std::vector<ArMember> mem;
    std::string why, s;
    const int rc = ar_parse(p, n, mem, why);
    for (const ArMember& m : mem) {
        for (unsigned char ch : m.name) { char h[3]; snprintf(h, sizeof h, "%02x", ch); s += h; }
        s += "\t" + std::to_string(m.off) + "\t" + std::to_string(m.size) + "\n";
    }
    snprintf(text, cap, "%s", s.c_str());
    return rc;
}

// the walker over a whole table, as the kernel runs it: verdicts[c] = (status, offset)
void sb_deflate_check(const uint8_t* in, uint64_t n_in, const uint8_t* z, const uint64_t* z_off, uint32_t nchunks, int last_is_final,
                      uint32_t* verdicts)
{
    InflateTables t;
    for (uint32_t c = 0; c < nchunks; ++c) {
        const DfCheckVerdict v = deflate_check_entry(in, n_in, z, z_off[nchunks], z_off, nullptr, c, last_is_final && c + 1 == nchunks, t);
        verdicts[2 * c] = v.status;
        verdicts[2 * c + 1] = v.offset;
    }
}

int sb_distance_ok(uint64_t dist, uint64_t front) { return df_check_distance_ok(dist, front) ? 1 : 0; }

} // extern "C"
