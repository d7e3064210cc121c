// Host harness for tests/test_snap_host.py: snappy_amd/csrc/snap_core.h compiled for the CPU -- the ar container, the
// choice of the member a call reads, and the audit's comparison of hashes.yaml with the tar headers, as snap.inc runs them.
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

std::vector<std::string> fields(const std::string& line)
{
    std::vector<std::string> f;
    std::stringstream ss(line);
    std::string x;
    while (std::getline(ss, x, '\t')) f.push_back(x);
    return f;
}

} // namespace

extern "C" {

// out: "name\toffset\tsize\n" per member, or the reason on failure
int sh_ar_parse(const uint8_t* p, uint64_t n, char* out, size_t cap)
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

// *index, *codec (0 gz, 1 bz2) of the member a call for `prefix` reads; why: the message on failure
int sh_ar_pick(const uint8_t* p, uint64_t n, const char* prefix, uint64_t* index, int* codec, char* why_out, size_t cap)
{
    std::vector<ArMember> mem;
    std::string why;
    int rc = ar_parse(p, n, mem, why);
    size_t i = 0;
    if (!rc) rc = ar_pick(mem, prefix, &i, codec, why);
    *index = i;
    put(why, why_out, cap);
    return rc;
}

// records: lines "name \t st_mode (octal) \t size or -1 \t sha512 hex or -"; members: lines "name \t type \t mode (octal)
// \t size \t digest hex or -".  -> 0 or the kind; the name in name_out.
int sh_audit(const char* records, const char* members, char* name_out, size_t cap)
{
    std::vector<AuditRecord> recs;
    std::vector<AuditMember> mem;
    std::vector<std::vector<uint8_t>> digs;
    std::stringstream rs(records), ms(members);
    std::string line;
    while (std::getline(rs, line)) {
        const auto f = fields(line);
        if (f.size() < 4) continue;
        AuditRecord r;
        r.name = f[0];
        r.st_mode = (uint32_t)strtoul(f[1].c_str(), nullptr, 8);
        r.has_size = f[2] != "-1";
        r.size = strtoll(f[2].c_str(), nullptr, 10);
        if (f[3] != "-") r.sha512_hex = f[3];
        recs.push_back(r);
    }
    std::vector<std::string> hexes;
    while (std::getline(ms, line)) {
        const auto f = fields(line);
        if (f.size() < 5) continue;
        AuditMember m;
        m.name = f[0];
        m.type = f[1][0];
        m.mode = (uint32_t)strtoul(f[2].c_str(), nullptr, 8);
        m.size = strtoull(f[3].c_str(), nullptr, 10);
        mem.push_back(m);
        hexes.push_back(f[4]);
    }
    digs.resize(mem.size());
    for (size_t k = 0; k < mem.size(); ++k) {
        if (hexes[k].size() != 128) continue;
        digs[k].resize(64);
        for (int i = 0; i < 64; ++i) digs[k][i] = (uint8_t)strtoul(hexes[k].substr(2 * i, 2).c_str(), nullptr, 16);
        mem[k].digest = digs[k].data();
    }
    std::string name;
    const int kind = snap_audit_compare(recs, mem, &name);
    put(name, name_out, cap);
    return kind;
}

} // extern "C"
