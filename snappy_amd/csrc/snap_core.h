// snap_core.h -- the parts of the .snap session that need neither a device nor the engine: the `ar` container (read, and
// written for snaphash_snap_build), the choice
// of the member a call reads (skipToArMember, clickdeb/deb.go:408-441) and the audit's comparison of hashes.yaml with the
// tar headers.  Host-only and self-contained, so that snap.inc and a host harness in tests/ run the same code.
//
// The container.  The reference reads it with an `ar` library that is not part of its tree, so what a member name is is
// defined here: the header's 16 name bytes with trailing spaces removed (nothing else is stripped -- a BSD/GNU trailing
// "/" stays; dpkg-deb and the reference's own writer produce none).  A GNU long-name table ("//") is not supported: its
// members keep the names "/<offset>", which match no prefix.  Layout: the global magic "!<arch>\n", then per member a
// 60-byte header -- name[16] mtime[12] uid[6] gid[6] mode[8] size[10] fmag[2] = "`\n", the size in decimal digits padded
// with spaces -- and the data, padded with one byte to an even offset.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/snaphash.h"

namespace snaphash {

struct ArMember {
    std::string name;
    uint64_t off = 0; // of the data, in the file
    uint64_t size = 0;
};

// The members of p[0..n).  0, or SNAPHASH_EFORMAT with the reason in why: a wrong global magic or fmag, a size field that
// is not decimal digits followed by spaces, a header the end of the file cuts off, a member that runs past it.  (The one
// padding byte after the LAST member may be missing, as ar readers accept.)
inline int ar_parse(const uint8_t* p, uint64_t n, std::vector<ArMember>& out, std::string& why)
{
    out.clear();
    if (n < 8 || memcmp(p, "!<arch>\n", 8) != 0) { why = "ar: not an ar archive (global magic)"; return SNAPHASH_EFORMAT; }
    uint64_t at = 8;
    while (at < n) {
        if (at + 60 > n) { why = "ar: truncated member header"; return SNAPHASH_EFORMAT; }
        const uint8_t* h = p + at;
        if (h[58] != '`' || h[59] != '\n') { why = "ar: bad member header magic"; return SNAPHASH_EFORMAT; }
        uint64_t size = 0;
        int i = 48;
        for (; i < 58 && h[i] >= '0' && h[i] <= '9'; ++i) size = size * 10 + (uint64_t)(h[i] - '0');
        bool ok = i > 48;
        for (; i < 58; ++i) ok = ok && h[i] == ' ';
        if (!ok) { why = "ar: bad member size field"; return SNAPHASH_EFORMAT; }
        size_t nl = 16;
        while (nl && h[nl - 1] == ' ') --nl;
        ArMember m;
        m.name.assign((const char*)h, nl);
        m.off = at + 60;
        m.size = size;
        if (size > n - m.off) { why = "ar: member " + m.name + " runs past the end of the file"; return SNAPHASH_EFORMAT; }
        out.push_back(m);
        at = m.off + size + (size & 1);
    }
    return 0;
}

// ---- the writer (snapbuild.inc: ClickDeb.Build, deb.go:381-403) --------------------------------------------------------------
// The reference's ar writer is not in its tree either, so what is written is defined here, field for field what ar_parse
// above (and ar(1), dpkg-deb) reads: the name left-justified in 16 bytes, the mtime in decimal in 12, uid "0" and gid "0" in
// 6 each, the mode in octal in 8, the size in decimal in 10 -- every field padded with spaces -- and "`\n".

constexpr char kArMagic[] = "!<arch>\n"; // 8 bytes
constexpr size_t kArHeader = 60;

// One member's header into out[60].  SNAPHASH_EINVAL: an empty name, one longer than 16 bytes or ending in a space (the
// reader would not give it back), a negative mtime, a number its field cannot hold.
inline int ar_header(const std::string& name, int64_t mtime, uint32_t mode, uint64_t size, uint8_t out[kArHeader])
{
    if (name.empty() || name.size() > 16 || name.back() == ' ') return SNAPHASH_EINVAL;
    if (mtime < 0 || mtime > 999999999999ll || mode > 077777777u || size > 9999999999ull) return SNAPHASH_EINVAL;
    memset(out, ' ', kArHeader);
    memcpy(out, name.data(), name.size());
    auto field = [&](size_t at, size_t width, uint64_t v, unsigned base) {
        char digits[24];
        size_t nd = 0;
        do { digits[nd++] = (char)('0' + v % base); v /= base; } while (v);
        for (size_t i = 0; i < nd && i < width; ++i) out[at + i] = (uint8_t)digits[nd - 1 - i];
    };
    field(16, 12, (uint64_t)mtime, 10);
    field(28, 6, 0, 10);
    field(34, 6, 0, 10);
    field(40, 8, mode, 8);
    field(48, 10, size, 10);
    out[58] = '`';
    out[59] = '\n';
    return 0;
}

struct ArInput {
    std::string name;
    const uint8_t* data = nullptr;
    uint64_t size = 0;
};

// A whole container in memory: the global magic, then header, data and the padding byte of every member.
inline int ar_write(const std::vector<ArInput>& mem, int64_t mtime, uint32_t mode, std::vector<uint8_t>& out)
{
    out.assign((const uint8_t*)kArMagic, (const uint8_t*)kArMagic + 8);
    for (const ArInput& m : mem) {
        uint8_t h[kArHeader];
        const int rc = ar_header(m.name, mtime, mode, m.size, h);
        if (rc) { out.clear(); return rc; }
        out.insert(out.end(), h, h + kArHeader);
        if (m.size) out.insert(out.end(), m.data, m.data + m.size);
        if (m.size & 1) out.push_back('\n');
    }
    return 0;
}

enum : int { kSnapGz = 0, kSnapBz2 = 1, kSnapXz = 2 };

// skipToArMember: the FIRST member whose name starts with prefix; its suffix picks the decoder.  0 with *index and *codec;
// SNAPHASH_EFORMAT when there is none (the reference: io.EOF from the ar reader); SNAPHASH_EINVAL -- what
// snaphash_tar_create answers to a name that is not ".gz" -- with the reference's text for any other suffix, and for ".xz"
// (an external tool upstream) unless xz_allowed: a session opened with SNAPHASH_SNAP_XZ takes it, codec kSnapXz.  Allowed or
// not, the first match decides: a ".xz" member in front of a ".gz" one is the member looked at.
inline int ar_pick_ex(const std::vector<ArMember>& mem, const std::string& prefix, bool xz_allowed, size_t* index, int* codec, std::string& why)
{
    for (size_t i = 0; i < mem.size(); ++i) {
        const std::string& nm = mem[i].name;
        if (nm.compare(0, prefix.size(), prefix) != 0) continue;
        *index = i;
        auto ends = [&](const char* s) { const size_t l = strlen(s); return nm.size() >= l && nm.compare(nm.size() - l, l, s) == 0; };
        if (ends(".gz")) { *codec = kSnapGz; return 0; }
        if (ends(".bz2")) { *codec = kSnapBz2; return 0; }
        if (xz_allowed && ends(".xz")) { *codec = kSnapXz; return 0; }
        why = "Can not handle " + nm;
        return SNAPHASH_EINVAL;
    }
    why = "ar: no " + prefix + " member";
    return SNAPHASH_EFORMAT;
}

// what snaphash_snap_open's sessions ask: ".xz" is refused
inline int ar_pick(const std::vector<ArMember>& mem, const std::string& prefix, size_t* index, int* codec, std::string& why)
{
    return ar_pick_ex(mem, prefix, false, index, codec, why);
}

// ---- the audit's comparison ----------------------------------------------------------------------------------------------

struct AuditRecord { // one record of hashes.yaml
    std::string name;
    uint32_t st_mode = 0; // POSIX type + permission bits (snaphash_mode_parse)
    bool has_size = false;
    int64_t size = 0;
    std::string sha512_hex;
};
struct AuditMember { // one tar member, name after filepath.Clean (a leading "./" is gone with it)
    std::string name;
    char type = '0';      // '0' regular, '2' symlink, '5' directory
    uint32_t mode = 0;    // the tar header's
    uint64_t size = 0;
    const uint8_t* digest = nullptr; // 64 raw bytes for the LAST regular member of a name, else null
};

inline bool audit_digest_is(const uint8_t* d, const std::string& hex)
{
    if (!d || hex.size() != 128) return false;
    for (int i = 0; i < 128; ++i) {
        const int v = (d[i / 2] >> ((i & 1) ? 0 : 4)) & 15;
        char ch = hex[i];
        if (ch >= 'A' && ch <= 'F') ch = (char)(ch - 'A' + 'a');
        if (ch != "0123456789abcdef"[v]) return false;
    }
    return true;
}

// hashes.yaml against the tar HEADERS (nothing is on disk in an audit), the first failure in this order:
//   the records in yaml order -- the LAST member of the record's name (whose content an unpack leaves on disk; an
//     EARLIER member of the name with another mode would leave its mode there, as UnpackTar's O_CREATE does -- that is
//     the unpack's Verify to find, the audit holds the record against the last header): none is kind 1;
//     the type letter or the low nine mode bits differ: kind 5; a regular file's size: kind 3, then its SHA-512: kind 4;
//   then the members in tar order: one whose name no record has is kind 2 (the archive's root entry "." is no member of
//     the tree: hashes.yaml never records the root).
// 0 = all agree; else the kind, the name in *name.
inline int snap_audit_compare(const std::vector<AuditRecord>& recs, const std::vector<AuditMember>& mem, std::string* name)
{
    std::unordered_map<std::string, size_t> last, recorded;
    for (size_t k = 0; k < mem.size(); ++k) last[mem[k].name] = k;
    for (size_t i = 0; i < recs.size(); ++i) {
        const AuditRecord& r = recs[i];
        recorded[r.name] = i;
        const auto it = last.find(r.name);
        *name = r.name;
        if (it == last.end()) return 1;
        const AuditMember& m = mem[it->second];
        const uint32_t fmt = r.st_mode & 0170000;
        const char want = fmt == 0040000 ? '5' : fmt == 0120000 ? '2' : '0';
        if (want != m.type || (r.st_mode & 0777) != (m.mode & 0777)) return 5;
        if (m.type != '0') continue;
        if (!r.has_size || r.size < 0 || (uint64_t)r.size != m.size) return 3;
        if (!audit_digest_is(m.digest, r.sha512_hex)) return 4;
    }
    for (const AuditMember& m : mem) {
        if (m.name == "." || recorded.count(m.name)) continue;
        *name = m.name;
        return 2;
    }
    name->clear();
    return 0;
}

} // namespace snaphash
