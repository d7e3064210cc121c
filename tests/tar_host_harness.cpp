// Host harness for tests/test_tar_host.py: snappy_amd/csrc/tar_core.h compiled for the CPU -- tar_read as unpack.inc and
// snap.inc run it, with the extent invariant its consumers rely on checked HERE on every call (tests/tar_sweep.h): a
// result that breaks it comes back as kInvariantBroken (77) whatever tar_read itself returned.
#include <stdio.h>

#include "tar_sweep.h"

using namespace snaphash;
using namespace tarsweep;

namespace {

void put(const std::string& s, char* out, size_t cap)
{
    if (!cap) return;
    const size_t k = std::min(s.size(), cap - 1);
    memcpy(out, s.data(), k);
    out[k] = 0;
}

std::string hex(const std::string& s) // (a name may hold any byte)
{
    std::string h;
    for (const unsigned char ch : s) { h += "0123456789abcdef"[ch >> 4]; h += "0123456789abcdef"[ch & 15]; }
    return h.empty() ? "-" : h;
}

} // namespace

extern "C" {

// tar_read over t[0..n).  out: a line "name(hex) \t type \t mode(octal) \t size \t data_off \t linkname(hex)" per entry
// appended (before a refusal too), then "reg" and the indices last_regular_members gives, then "why" and the reason.
// -> tar_read's code, or 77 when an entry's extent leaves the stream.
int th_tar_read(const uint8_t* t, uint64_t n, char* out, size_t cap)
{
    std::vector<TarEntry> ents;
    std::string why, s;
    const int rc = read_checked(t, n, ents, why);
    char num[96];
    for (const TarEntry& e : ents) {
        snprintf(num, sizeof num, "\t%c\t%o\t%llu\t%llu\t", e.type, e.mode, (unsigned long long)e.size, (unsigned long long)e.data_off);
        s += hex(e.name) + num + hex(e.linkname) + "\n";
    }
    s += "reg";
    if (rc != kInvariantBroken)
        for (const size_t k : last_regular_members(ents)) s += "\t" + std::to_string(k);
    s += "\nwhy\t" + why + "\n";
    put(s, out, cap);
    return rc;
}

// The mutation sweep over one archive.  regions: triples (offset, length, 1 for a header block / 0 for a PAX or GNU body);
// every stride-th bit of each flipped, then every numeric field of each header set to its four values.  *runs: calls of
// tar_read made.  -> 0, or 77 with the byte offset of the mutation in *where.
int th_sweep(const uint8_t* t, uint64_t n, const uint64_t* regions, size_t n_regions, uint64_t stride, uint64_t* runs, uint64_t* where)
{
    Sweep sw;
    sw.buf.assign(t, t + n);
    bool ok = true;
    for (size_t r = 0; ok && r < n_regions; ++r) {
        ok = sw.bits(regions[3 * r], regions[3 * r + 1], regions[3 * r + 2] != 0, stride ? stride : 1);
        if (ok && regions[3 * r + 2]) ok = sw.fields(regions[3 * r]);
    }
    *runs = sw.runs;
    *where = sw.broken_at;
    return ok ? 0 : kInvariantBroken;
}

int th_go_clean(const char* p, size_t n, char* out, size_t cap)
{
    put(go_clean(std::string(p, n)), out, cap);
    return 0;
}

} // extern "C"
