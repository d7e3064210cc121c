// Host harness for tests/test_snap_xz_host.py: the parts of snappy_amd/csrc/snap_core.h that the .xz route of the .snap
// session and the codec of snaphash_snap_build added or lean on -- the member lookup with ".xz" allowed (ar_pick_ex) beside
// the one that refuses it (ar_pick), and the container's writer with the data member's three names.
#include <stdio.h>
#include <stdlib.h>

#include <sstream>

#include "../snappy_amd/csrc/snap_core.h"

using namespace snaphash;

namespace {

void put(const std::string& s, char* out, size_t cap)
{
    if (cap) snprintf(out, cap, "%s", s.c_str());
}

} // namespace

extern "C" {

// ar_pick_ex (xz_allowed != 0) or ar_pick itself (xz_allowed < 0: the wrapper, not the variant with false) over the members
// of p[0..n): *index, *codec (0 gz, 1 bz2, 2 xz); why: the message on failure
int sx_ar_pick(const uint8_t* p, uint64_t n, const char* prefix, int xz_allowed, uint64_t* index, int* codec, char* why_out, size_t cap)
{
    std::vector<ArMember> mem;
    std::string why;
    int rc = ar_parse(p, n, mem, why);
    size_t i = 0;
    if (!rc) rc = xz_allowed < 0 ? ar_pick(mem, prefix, &i, codec, why) : ar_pick_ex(mem, prefix, xz_allowed != 0, &i, codec, why);
    *index = i;
    put(why, why_out, cap);
    return rc;
}

// ar_write of the members in `spec` -- lines "name \t size", member k's data being `size` bytes of the value 'a' + k -- with
// one mtime and mode; out receives the container, *out_len its length.  -> ar_write's code, or -100 when out is too small.
int sx_ar_write(const char* spec, int64_t mtime, uint32_t mode, uint8_t* out, size_t cap, size_t* out_len)
{
    std::vector<std::vector<uint8_t>> datas;
    std::vector<std::string> names;
    std::stringstream ss(spec);
    std::string line;
    while (std::getline(ss, line)) {
        const size_t tab = line.find('\t');
        if (tab == std::string::npos) continue;
        names.push_back(line.substr(0, tab));
        datas.emplace_back((size_t)strtoull(line.c_str() + tab + 1, nullptr, 10), (uint8_t)('a' + datas.size()));
    }
    std::vector<ArInput> in(names.size());
    for (size_t k = 0; k < names.size(); ++k) in[k] = ArInput{names[k], datas[k].data(), datas[k].size()};
    std::vector<uint8_t> ar;
    const int rc = ar_write(in, mtime, mode, ar);
    *out_len = ar.size();
    if (rc) return rc;
    if (ar.size() > cap) return -100;
    memcpy(out, ar.data(), ar.size());
    return 0;
}

// ar_header alone: 60 bytes into out
int sx_ar_header(const char* name, int64_t mtime, uint32_t mode, uint64_t size, uint8_t* out) { return ar_header(name, mtime, mode, size, out); }

// ar_parse: "name\toffset\tsize\n" per member, or the reason on failure
int sx_ar_parse(const uint8_t* p, uint64_t n, char* out, size_t cap)
{
    std::vector<ArMember> mem;
    std::string why;
    const int rc = ar_parse(p, n, mem, why);
    if (rc) { put(why, out, cap); return rc; }
    std::string s;
    for (const ArMember& m : mem) s += m.name + "\t" + std::to_string(m.off) + "\t" + std::to_string(m.size) + "\n";
    put(s, out, cap);
    return 0;
}

} // extern "C"
