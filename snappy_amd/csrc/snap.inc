// snap.inc -- the .snap itself, textually part of snaphash_api.cpp (after unpack.inc, unbz2.inc and unxz.inc: it owns the
// session and drives their codecs, tar reader, member writer and Verify tail; DecodedStream owns what is in c->inf.d_out).
//
// The reference opens a package with ClickDeb.Open (clickdeb/deb.go:108-127) and reads it through an `ar` reader:
// ControlMember / MetaMember (deb.go:141-183) decode a whole tar to fetch one file, Unpack (deb.go:188-203) decodes
// data.tar.* again.  Here a session reads the file once, parses the container (snap_core.h), and decodes each of the two
// tars at most once: the decoded stream and its member list stay in the session, the data.tar stream in c->inf.d_out too
// for the in-pass Verify and the audit.  Another decode on the ctx may take that buffer (control.tar.* after a
// MetaMember call does): the engine counts the decodes that wrote it (DevCtx::fout_gen), and a session whose stream is no
// longer there copies it up again from host memory -- it is never decoded twice.  All of this is blind to the codec: a
// member goes to the decoder its suffix names (kSnapCodecs), ".xz" only in a session opened with SNAPHASH_SNAP_XZ
// (snaphash_snap_open_ex), which then takes the chains SNAPHASH_UNXZ_BCJ takes (DESIGN.md sec. 28).

#include "tar_core.h"

struct snaphash_snap {
    snaphash_ctx* x = nullptr;
    std::string path;
    std::vector<uint8_t> file;
    std::vector<ArMember> mem;
    bool xz = false; // SNAPHASH_SNAP_XZ: ".xz" members go to kUnxzCodec
    bool xz_chains = false; // SNAPHASH_SNAP_XZ_CHAINS: and may carry every chain SNAPHASH_UNXZ_CHAINS takes
    struct Tar {
        bool tried = false;
        int rc = 0;            // of the decode and tar_read
        std::string err;
        size_t member = 0;     // index into mem
        std::vector<uint8_t> tar;
        std::vector<TarEntry> ents;
        snaphash_unpack_stats st{};
        uint8_t adig[64] = {0}; // SHA-512 of the member's bytes
        uint64_t gen = 0;       // DevCtx::fout_gen when the stream was left in c->inf.d_out
    } control, data;
    snaphash_snap_stats stats{};
    CrcTally tally;
};

namespace {

const UnpackCodec* const kSnapCodecs[] = {&kGunzipCodec, &kBunzip2Codec, &kUnxzCodec}; // by ar_pick_ex's codec (snap_core.h)
static_assert(kSnapGz == 0 && kSnapBz2 == 1 && kSnapXz == 2, "kSnapCodecs is indexed by ar_pick_ex's codec");

// The tar behind `prefix`, decoded once: t.rc / t.err keep what came of it for every later call.
int snap_tar(snaphash_snap* s, snaphash_snap::Tar& t, const char* prefix, bool keep_dev)
{
    snaphash_ctx* x = s->x;
    DevCtx* c = x->d0();
    if (t.tried) return t.rc ? fail(x, t.rc, t.err) : 0;
    t.tried = true;
    int codec = 0;
    std::string why;
    t.rc = ar_pick_ex(s->mem, prefix, s->xz, &t.member, &codec, why);
    if (t.rc) { t.err = why; return fail(x, t.rc, t.err); }
    const uint8_t* z = s->file.data() + s->mem[t.member].off;
    const size_t zn = (size_t)s->mem[t.member].size;
    t.st = snaphash_unpack_stats{};
    t.st.struct_size = sizeof t.st;
    t.st.gz_bytes = zn;
    const double t0 = now_ms();
    {
        DigestThread dig_th(z, zn, t.adig);
        DecodedStream ds(c, t.tar, keep_dev);
        UnxzCall xz_call(x); // an .xz member: one BCJ filter in front of LZMA2 is taken, as the xz tool the reference pipes through takes it
        if (codec == kSnapXz) xz_call.allow_bcj();
        if (codec == kSnapXz && s->xz_chains) xz_call.allow_chains();
        // under SNAPHASH_FLAG_GPU_ONLY the stream reaches HBM before host memory: the CRCs are taken there
        t.rc = kSnapCodecs[codec]->decode(x, c, z, zn, ds, t.st, x->gpu_only ? CrcAt::Device : CrcAt::Host, &s->tally);
        scratch_spans_done(c);
    }
    (&t == &s->data ? s->stats.data_decodes : s->stats.control_decodes)++;
    s->stats.device_crc_ranges = s->tally.device_ranges;
    s->stats.host_crc_ranges = s->tally.host_ranges;
    s->stats.device_crc_ms = s->tally.device_ms;
    t.gen = c->fout_gen;
    t.st.tar_bytes = t.tar.size();
    if (t.rc) { t.err = c->last_error; return lift(x, c, t.rc); }
    t.rc = tar_read(t.tar.data(), t.tar.size(), t.ents, why);
    t.st.members = t.ents.size();
    t.st.wall_ms = now_ms() - t0;
    if (t.rc) { t.err = why; return fail(x, t.rc, t.err); }
    return 0;
}

// member(): the content of the LAST tar member whose cleaned name is `want` (deb.go:167-176)
int snap_member(snaphash_snap* s, snaphash_snap::Tar& t, const std::string& want, void** content, size_t* len)
{
    *content = nullptr;
    *len = 0;
    const TarEntry* hit = nullptr;
    for (const TarEntry& e : t.ents)
        if (e.name == want) hit = &e;
    if (!hit) return SNAPHASH_OK;
    if (hit->data_off > t.tar.size() || hit->size > t.tar.size() - hit->data_off) return fail(s->x, SNAPHASH_EFORMAT, "tar: member outside the stream");
    void* p = malloc(hit->size ? (size_t)hit->size : 1);
    if (!p) return fail(s->x, SNAPHASH_ENOMEM, "malloc");
    if (hit->size) memcpy(p, t.tar.data() + hit->data_off, (size_t)hit->size);
    *content = p;
    *len = (size_t)hit->size;
    return SNAPHASH_OK;
}

// the package's own hashes.yaml out of control.tar.*; *yaml stays null when there is none
int snap_yaml(snaphash_snap* s, const uint8_t** yaml, size_t* yaml_len)
{
    *yaml = nullptr;
    int rc = snap_tar(s, s->control, "control.tar", false);
    if (rc) return rc;
    for (const TarEntry& e : s->control.ents)
        if (e.name == "hashes.yaml" && e.type == '0') { *yaml = s->control.tar.data() + e.data_off; *yaml_len = (size_t)e.size; }
    return 0;
}

// the data.tar stream in c->inf.d_out again if another decode has written there since
int snap_data_on_device(snaphash_snap* s)
{
    DevCtx* c = s->x->d0();
    if (s->data.gen == c->fout_gen && c->inf.d_out.size() >= s->data.tar.size()) return 0;
    const int rc = DecodedStream::upload(c, s->data.tar);
    if (rc) return rc;
    s->data.gen = ++c->fout_gen;
    return 0;
}

#define SNAP_ENTER(s)                                                            \
    if (!(s) || !(s)->x) return SNAPHASH_EINVAL;                                 \
    snaphash_ctx* x = (s)->x;                                                    \
    TOP_ENTER(x);                                                                \
    DevCtx* c = x->d0();                                                         \
    HIP_TRY(c, hipSetDevice(c->device))

} // namespace

extern "C" {

int snaphash_snap_open(snaphash_ctx* x, const char* snap_path, snaphash_snap** out) { return snaphash_snap_open_ex(x, snap_path, nullptr, out); }

int snaphash_snap_open_ex(snaphash_ctx* x, const char* snap_path, const snaphash_snap_open_options* opt, snaphash_snap** out)
try {
    if (!x || !snap_path || !out) return fail(x, SNAPHASH_EINVAL, "bad argument");
    *out = nullptr;
    uint32_t flags = 0;
    if (opt && (opt->struct_size || opt->flags)) { // (all zero: snaphash_snap_open)
        if (opt->struct_size < sizeof(snaphash_snap_open_options)) return fail(x, SNAPHASH_EINVAL, "snaphash_snap_open_options.struct_size");
        if (opt->flags & ~(uint32_t)(SNAPHASH_SNAP_XZ | SNAPHASH_SNAP_XZ_CHAINS)) return fail(x, SNAPHASH_EINVAL, "snap: unknown flag");
        if ((opt->flags & SNAPHASH_SNAP_XZ_CHAINS) && !(opt->flags & SNAPHASH_SNAP_XZ)) return fail(x, SNAPHASH_EINVAL, "snap: SNAPHASH_SNAP_XZ_CHAINS needs SNAPHASH_SNAP_XZ");
        flags = opt->flags;
    }
    std::unique_ptr<snaphash_snap> s(new snaphash_snap);
    s->x = x;
    s->xz = (flags & SNAPHASH_SNAP_XZ) != 0;
    s->xz_chains = (flags & SNAPHASH_SNAP_XZ_CHAINS) != 0;
    s->path = snap_path;
    s->stats.struct_size = sizeof s->stats;
    int rc = read_whole(x, snap_path, s->file);
    if (rc) return rc;
    std::string why;
    rc = ar_parse(s->file.data(), s->file.size(), s->mem, why);
    if (rc) return fail(x, rc, std::string(snap_path) + ": " + why);
    *out = s.release();
    return SNAPHASH_OK;
} catch (...) {
    return SNAPHASH_ENOMEM;
}

void snaphash_snap_close(snaphash_snap* s) { delete s; }

size_t snaphash_snap_members(const snaphash_snap* s) { return s ? s->mem.size() : 0; }

int snaphash_snap_member_info(const snaphash_snap* s, size_t i, const char** name, uint64_t* offset, uint64_t* size)
{
    if (!s || i >= s->mem.size()) return SNAPHASH_EINVAL;
    if (name) *name = s->mem[i].name.c_str();
    if (offset) *offset = s->mem[i].off;
    if (size) *size = s->mem[i].size;
    return SNAPHASH_OK;
}

int snaphash_snap_control_member(snaphash_snap* s, const char* name, void** content, size_t* len)
try {
    if (!s || !name || !content || !len) return SNAPHASH_EINVAL;
    SNAP_ENTER(s);
    (void)t_top0_;
    const int rc = snap_tar(s, s->control, "control.tar", false);
    if (rc) return rc;
    return snap_member(s, s->control, name, content, len);
} catch (...) {
    return SNAPHASH_ENOMEM;
}

int snaphash_snap_meta_member(snaphash_snap* s, const char* name, void** content, size_t* len)
try {
    if (!s || !name || !content || !len) return SNAPHASH_EINVAL;
    SNAP_ENTER(s);
    (void)t_top0_;
    const int rc = snap_tar(s, s->data, "data.tar", true);
    if (rc) return rc;
    return snap_member(s, s->data, go_clean(std::string("meta/") + name), content, len); // filepath.Join cleans
} catch (...) {
    return SNAPHASH_ENOMEM;
}

int snaphash_snap_unpack(snaphash_snap* s, const char* target_dir, int verify, snaphash_mismatch* first, uint8_t* archive_digest)
try {
    if (!s || !target_dir) return SNAPHASH_EINVAL;
    SNAP_ENTER(s);
    const uint8_t* yaml = nullptr;
    size_t yaml_len = 0;
    int rc = 0;
    if (verify) {
        rc = snap_yaml(s, &yaml, &yaml_len);
        if (rc) return rc;
        if (!yaml) return mismatch(x, first, 1, "hashes.yaml");
    }
    rc = snap_tar(s, s->data, "data.tar", true);
    snaphash_unpack_stats st = s->data.st;
    if (archive_digest && s->data.tried && s->data.member < s->mem.size()) memcpy(archive_digest, s->data.adig, 64);
    if (!rc) rc = lift(x, c, unpack_members(c, s->data.ents, s->data.tar.data(), target_dir));
    if (!rc && verify) {
        rc = snap_data_on_device(s);
        if (!rc) rc = verify_unpacked(x, c, s->data.tar, s->data.ents, target_dir, s->path.c_str(), s->data.adig, (const char*)yaml, yaml_len, first);
    }
    st.wall_ms = now_ms() - t_top0_;
    x->unpack = st;
    end_top(x, t_top0_);
    return rc;
} catch (...) {
    return SNAPHASH_ENOMEM;
}

int snaphash_snap_audit(snaphash_snap* s, snaphash_mismatch* first, uint8_t* archive_digest)
try {
    if (!s) return SNAPHASH_EINVAL;
    SNAP_ENTER(s);
    const uint8_t* yaml = nullptr;
    size_t yaml_len = 0;
    int rc = snap_yaml(s, &yaml, &yaml_len);
    if (rc) return rc;
    if (!yaml) return mismatch(x, first, 1, "hashes.yaml");
    rc = snap_tar(s, s->data, "data.tar", true);
    if (s->data.tried && s->data.member < s->mem.size() && archive_digest) memcpy(archive_digest, s->data.adig, 64);
    if (rc) return rc;
    x->unpack = s->data.st;
    ParsedHashes ph;
    rc = parse_yaml((const char*)yaml, yaml_len, ph);
    if (rc) return fail(x, rc, "hashes.yaml: parse error");
    if (!ph.has_archive || !digest_matches_hex(s->data.adig, ph.archive_hex)) return mismatch(x, first, 6, "archive-sha512");
    rc = snap_data_on_device(s);
    if (rc) return lift(x, c, rc);
    const std::vector<TarEntry>& ents = s->data.ents;
    const std::vector<size_t> reg = last_regular_members(ents);
    std::vector<uint8_t> dig;
    rc = hash_members(x, c, s->data.tar, ents, reg, dig);
    if (rc) return rc;
    std::vector<AuditMember> mem(ents.size());
    for (size_t k = 0; k < ents.size(); ++k) {
        mem[k].name = ents[k].name;
        mem[k].type = ents[k].type;
        mem[k].mode = ents[k].mode;
        mem[k].size = ents[k].size;
    }
    for (size_t q = 0; q < reg.size(); ++q) mem[reg[q]].digest = dig.data() + 64 * q;
    std::vector<AuditRecord> recs(ph.files.size());
    for (size_t i = 0; i < recs.size(); ++i) {
        recs[i].name = ph.files[i].name;
        recs[i].st_mode = ph.files[i].st_mode;
        recs[i].has_size = ph.files[i].has_size;
        recs[i].size = ph.files[i].size;
        recs[i].sha512_hex = ph.files[i].sha512_hex;
    }
    std::string name;
    const int kind = snap_audit_compare(recs, mem, &name);
    end_top(x, t_top0_);
    return kind ? mismatch(x, first, kind, name) : SNAPHASH_OK;
} catch (...) {
    return SNAPHASH_ENOMEM;
}

int snaphash_snap_get_stats(const snaphash_snap* s, snaphash_snap_stats* out)
{
    if (!s || !out || out->struct_size < sizeof(snaphash_snap_stats)) return SNAPHASH_EINVAL;
    *out = s->stats;
    out->struct_size = sizeof(snaphash_snap_stats);
    return SNAPHASH_OK;
}

} // extern "C"
