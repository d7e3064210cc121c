// tar_core.h -- the tar reader of the install side: archive/tar's Reader as helpers.UnpackTar drives it with
// clickVerifyContentFn (clickdeb/deb.go:96-103, helpers/helpers.go:104-147).  Host-only and self-contained (the standard
// library alone), so that unpack.inc, snap.inc and a host harness in tests/ run the same code.
//
// What tar_read promises its consumers -- the member writer, the session's member() and, through the SHA-512 job tables of
// hash_members, the kernels that read the decoded stream in HBM with no check of their own:
//
//     every entry appended has data_off <= n and size <= n - data_off
//
// whatever the stream holds, for entries appended before a refusal too.  Every number read from the stream is compared
// with what is LEFT of the stream (`x > n - at`), never added to an offset first: a sum can wrap, the difference cannot.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

namespace snaphash {

// the values of SNAPHASH_EFORMAT and SNAPHASH_ECONTENT (include/snaphash.h; unpack.inc asserts that they are)
enum : int { kTarEFormat = -9, kTarEContent = -10 };

struct TarEntry {
    std::string name;     // after clickVerifyContentFn (filepath.Clean)
    std::string linkname;
    char type = '0';
    uint32_t mode = 0;    // permission and set-id bits
    uint64_t size = 0;
    uint64_t data_off = 0;
};

// Go's filepath.Clean (path/filepath, Unix)
inline std::string go_clean(const std::string& p)
{
    if (p.empty()) return ".";
    const bool rooted = p[0] == '/';
    std::vector<std::string> parts;
    size_t i = 0;
    while (i < p.size()) {
        size_t j = p.find('/', i);
        if (j == std::string::npos) j = p.size();
        const std::string e = p.substr(i, j - i);
        i = j + 1;
        if (e.empty() || e == ".") continue;
        if (e == "..") {
            if (!parts.empty() && parts.back() != "..") parts.pop_back();
            else if (!rooted) parts.push_back("..");
            continue;
        }
        parts.push_back(e);
    }
    std::string r = rooted ? "/" : "";
    for (size_t k = 0; k < parts.size(); ++k) r += (k ? "/" : "") + parts[k];
    return r.empty() ? "." : r;
}

// A numeric header field (archive/tar's parseNumeric): octal digits between blanks and NULs, or base-256 behind a first
// byte with bit 7 set.  false for anything else, for a value of 2^63 or more, and for a NEGATIVE base-256 value (bit 6 of
// the first byte: two's complement) -- in every field, the mode included: no member of a package has one.
inline bool tar_octal(const uint8_t* f, size_t w, uint64_t* v)
{
    if (f[0] & 0x80) {
        if (f[0] & 0x40) return false;
        uint64_t x = f[0] & 0x3f;
        for (size_t i = 1; i < w; ++i) { if (x >> 55) return false; x = x << 8 | f[i]; }
        *v = x;
        return true;
    }
    size_t i = 0;
    while (i < w && (f[i] == ' ' || f[i] == 0)) ++i;
    uint64_t x = 0;
    for (; i < w && f[i] >= '0' && f[i] <= '7'; ++i) { if (x >> 60) return false; x = x * 8 + (f[i] - '0'); }
    for (; i < w; ++i) if (f[i] != ' ' && f[i] != 0) return false;
    *v = x;
    return true;
}

inline std::string tar_str(const uint8_t* f, size_t w)
{
    size_t k = 0;
    while (k < w && f[k]) ++k;
    return std::string((const char*)f, k);
}

// A number of a PAX record (its length, the value of "size"): decimal digits only, the whole of s[0..len), at least one,
// and no more than 2^63-1 (archive/tar parses them as int64).
inline bool tar_pax_number(const char* s, size_t len, uint64_t* v)
{
    if (len == 0) return false;
    uint64_t x = 0;
    for (size_t i = 0; i < len; ++i) {
        if (s[i] < '0' || s[i] > '9') return false;
        const uint64_t d = (uint64_t)(s[i] - '0');
        if (x > (((uint64_t)1 << 63) - 1 - d) / 10) return false;
        x = x * 10 + d;
    }
    *v = x;
    return true;
}

// The members of the tar stream t[0..n).  0; kTarEFormat (SNAPHASH_EFORMAT) for a stream archive/tar refuses;
// kTarEContent (SNAPHASH_ECONTENT) for a name with ".." or a member type UnpackTar does not create.  Entries read before a
// refusal stay in ents.  The extent promise is in the file comment.
//
// The project's own choices, where the reference's reader would go on: a PAX global header ('g') is ECONTENT; nothing
// behind the second zero block is looked at; a member whose data reaches the end of the stream but whose padding does not
// is refused, and so is an 'x', 'L' or 'K' with no member behind it (both as Python's tarfile does); a rooted name is
// kept rooted here -- the writer joins it under the target, as filepath.Join does.  An 'L'/'K' and an 'x' in front of one member: the one that comes FIRST names it (archive/tar of the
// reference's time and tarfile both read the next header recursively, so the outer one is applied last).
inline int tar_read(const uint8_t* t, uint64_t n, std::vector<TarEntry>& ents, std::string& why)
{
    uint64_t at = 0;
    std::string pax_path, pax_link, gnu_name, gnu_link;
    bool pax_size = false, gnu_name_first = false, gnu_link_first = false;
    bool meta_pending = false; // an 'x', 'L' or 'K' was read and the member it describes was not yet
    uint64_t pax_sz = 0;
    static const uint8_t zero[512] = {0};
    for (;;) {
        if (at == n || (n - at >= 512 && !memcmp(t + at, zero, 512))) {
            if (meta_pending) { why = "tar: the archive ends behind an extended header"; return kTarEFormat; }
            if (at == n) return 0; // (io.EOF at a record boundary)
        }
        if (n - at < 512) { why = "tar: truncated header"; return kTarEFormat; }
        const uint8_t* hd = t + at;
        if (!memcmp(hd, zero, 512)) {
            if (n - at >= 1024 && memcmp(hd + 512, zero, 512)) { why = "tar: invalid header"; return kTarEFormat; }
            return 0;
        }
        uint64_t chk = 0;
        if (!tar_octal(hd + 148, 8, &chk)) { why = "tar: invalid header"; return kTarEFormat; }
        int64_t su = 0, ss = 0;
        for (int i = 0; i < 512; ++i) {
            const uint8_t b = (i >= 148 && i < 156) ? ' ' : hd[i];
            su += b;
            ss += (int8_t)b;
        }
        if ((int64_t)chk != su && (int64_t)chk != ss) { why = "tar: header checksum"; return kTarEFormat; }
        uint64_t size = 0, mode = 0;
        if (!tar_octal(hd + 124, 12, &size) || !tar_octal(hd + 100, 8, &mode)) { why = "tar: invalid header"; return kTarEFormat; }
        const char type = (char)hd[156];
        const bool meta = type == 'x' || type == 'L' || type == 'K';
        if (pax_size && !meta) size = pax_sz; // (of the member the record precedes: an 'L', 'K' or 'x' between has its own)
        const uint64_t data = at + 512;       // <= n
        const bool has_data = type == '0' || type == 0 || type == '7' || meta || type == 'g';
        if (!has_data) size = 0; // (links, devices, directories: no content)
        if (size > n - data) { why = "tar: truncated member"; return kTarEFormat; }
        const uint64_t padded = (size + 511) & ~(uint64_t)511; // (size <= n: no wrap)
        if (padded > n - data) { why = "tar: truncated member"; return kTarEFormat; }
        if (meta) {
            const char* body = (const char*)t + data;
            const size_t bn = (size_t)size;
            if (type == 'L') { gnu_name = tar_str((const uint8_t*)body, bn); gnu_name_first = pax_path.empty(); }
            else if (type == 'K') { gnu_link = tar_str((const uint8_t*)body, bn); gnu_link_first = pax_link.empty(); }
            else { // records "<len> <key>=<value>\n" (archive/tar parsePAX)
                const auto bad = [&] { why = "tar: invalid PAX record"; return kTarEFormat; };
                size_t p = 0;
                while (p < bn) {
                    const char* sp = (const char*)memchr(body + p, ' ', bn - p);
                    if (!sp) return bad();
                    const size_t nd = (size_t)(sp - (body + p)); // digits of the length
                    uint64_t len = 0;
                    if (!tar_pax_number(body + p, nd, &len)) return bad();
                    if (len < nd + 4 || len > bn - p || body[p + len - 1] != '\n') return bad(); // at least "<len> k=\n"
                    const char* kv = sp + 1;
                    const size_t kvn = (size_t)len - nd - 2;
                    const char* eq = (const char*)memchr(kv, '=', kvn);
                    if (!eq || eq == kv) return bad();
                    const std::string k(kv, (size_t)(eq - kv)), v(eq + 1, kvn - (size_t)(eq + 1 - kv));
                    if (k.find('\0') != std::string::npos) return bad();
                    if (k == "path" || k == "linkpath") {
                        if (v.find('\0') != std::string::npos) return bad(); // (as archive/tar's validPAXRecord)
                        (k == "path" ? pax_path : pax_link) = v;
                    } else if (k == "size") {
                        if (!tar_pax_number(v.data(), v.size(), &pax_sz)) return bad();
                        pax_size = true;
                    }
                    p += (size_t)len;
                }
            }
            meta_pending = true;
            at = data + padded;
            continue;
        }
        TarEntry e;
        std::string name = tar_str(hd, 100);
        if (!memcmp(hd + 257, "ustar", 5)) {
            const std::string prefix = tar_str(hd + 345, 155);
            if (!prefix.empty()) name = prefix + "/" + name;
        }
        if (!gnu_name.empty() && !pax_path.empty()) name = gnu_name_first ? gnu_name : pax_path;
        else if (!gnu_name.empty()) name = gnu_name;
        else if (!pax_path.empty()) name = pax_path;
        e.linkname = tar_str(hd + 157, 100);
        if (!gnu_link.empty() && !pax_link.empty()) e.linkname = gnu_link_first ? gnu_link : pax_link;
        else if (!gnu_link.empty()) e.linkname = gnu_link;
        else if (!pax_link.empty()) e.linkname = pax_link;
        pax_path.clear(); pax_link.clear(); gnu_name.clear(); gnu_link.clear();
        pax_size = meta_pending = false;
        e.name = go_clean(name);
        if (e.name.find("..") != std::string::npos) { why = "tar: " + name + ": invalid content"; return kTarEContent; }
        e.type = type == 0 || type == '7' ? '0' : type;
        if (e.type != '0' && e.type != '2' && e.type != '5') { why = "tar: " + name + ": unsupported member type"; return kTarEContent; }
        e.mode = (uint32_t)(mode & 07777);
        e.size = size; // (0 for a directory or a link)
        e.data_off = data;
        ents.push_back(e);
        at = data + padded;
    }
}

// the last member of every name that is a regular file (the content an unpack leaves on disk), ascending
inline std::vector<size_t> last_regular_members(const std::vector<TarEntry>& ents)
{
    std::unordered_map<std::string, size_t> last;
    for (size_t k = 0; k < ents.size(); ++k) last[ents[k].name] = k;
    std::vector<size_t> reg;
    for (const auto& kv : last)
        if (ents[kv.second].type == '0') reg.push_back(kv.second);
    std::sort(reg.begin(), reg.end());
    return reg;
}

} // namespace snaphash
