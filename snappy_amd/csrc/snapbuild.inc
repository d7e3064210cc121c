// snapbuild.inc -- writing the .snap, textually part of snaphash_api.cpp (after targz.inc, xzpack.inc and bzpack.inc, whose
// producers it drives, and snap.inc, whose container it writes).
//
// ClickDeb.Build (reference clickdeb/deb.go:346-406) runs tarCreate over the tree into a temporary data.tar.gz, calls
// snappy.Build's callback -- writeHashes (snappy/build.go:216-270), which reads the archive and every file a second time --
// runs tarCreate over DEBIAN/ into control.tar.gz, and hands four members to an `ar` writer.  Here the first three steps
// are the fused pass of targz.inc (every source file read once: tar, DEFLATE, per-file SHA-512 and the archive digest),
// then that pass again over DEBIAN/ with buffers sized for the job, then the container (snap_core.h).  control.tar.gz
// comes before data.tar.gz in the container and holds the data member's digest, so the data member waits in a temporary
// file beside the target -- not in host memory: a member is as large as the package, and the file's pages are the
// page cache's to keep or drop -- until the control member is known; the copy into the container feeds the file's own
// SHA-512 (the store's download_sha512), so the .snap is not read back for it.  The reference hard-codes data.tar.gz "for
// distros like trusty that does not support xz yet" (deb.go:359); here the data member's Encoder is the caller's choice
// (snaphash_snap_build_options.data_codec: GzipEncoder, XzEncoder or BzEncoder through the same tar_create_impl), the
// control member stays gzip (DESIGN.md sec. 28).

namespace {

constexpr uint32_t kSnapBuildOptionsSizeV1 = 16; // snaphash_snap_build_options before data_codec, reserved, xz and bz2

struct SnapBuildTemps { // removed on every way out
    std::string data, control;
    ~SnapBuildTemps()
    {
        if (!data.empty()) (void)unlink(data.c_str());
        if (!control.empty()) (void)unlink(control.c_str());
    }
};

struct SnapOut {
    int fd = -1;
    HostSha sha;
    uint64_t bytes = 0;
    ~SnapOut() { if (fd >= 0) close(fd); }
    int put(const uint8_t* p, size_t n) // -> 0 or an errno
    {
        host_sha512_update(sha, p, n);
        bytes += n;
        size_t off = 0;
        while (off < n) {
            const ssize_t w = write(fd, p + off, n - off);
            if (w < 0) { if (errno == EINTR) continue; return errno; }
            off += (size_t)w;
        }
        return 0;
    }
};

// one member: header, data (from memory, or the whole of the file `path`), padding
int snap_put_member(snaphash_ctx* x, SnapOut& out, const char* name, int64_t mtime, const uint8_t* data, uint64_t size, const char* path)
{
    int fd = -1;
    struct FdGuard { int& fd; ~FdGuard() { if (fd >= 0) close(fd); } } guard{fd};
    if (path) {
        fd = open(path, O_RDONLY | O_CLOEXEC);
        struct stat sb;
        if (fd < 0 || fstat(fd, &sb) != 0) return fail(x, SNAPHASH_EIO, std::string(path) + ": " + strerror(errno));
        size = (uint64_t)sb.st_size;
    }
    uint8_t h[kArHeader];
    int rc = ar_header(name, mtime, 0100644, size, h);
    if (rc) return fail(x, rc, std::string("ar: member ") + name + " does not fit a header");
    int en = out.put(h, sizeof h);
    if (!en && !path && size) en = out.put(data, (size_t)size);
    if (!en && path) {
        std::vector<uint8_t> buf(4u << 20);
        uint64_t got = 0;
        while (got < size && !en) {
            const ssize_t r = read(fd, buf.data(), (size_t)std::min<uint64_t>(buf.size(), size - got));
            if (r < 0 && errno == EINTR) continue;
            if (r <= 0) return fail(x, SNAPHASH_EIO, std::string(path) + ": " + (r < 0 ? strerror(errno) : "shorter than it was"));
            en = out.put(buf.data(), (size_t)r);
            got += (uint64_t)r;
        }
    }
    if (!en && (size & 1)) en = out.put((const uint8_t*)"\n", 1);
    if (en) return fail(x, SNAPHASH_EIO, std::string("writing the container: ") + strerror(en));
    return SNAPHASH_OK;
}

// The data member of one build: its producer, made by the entry with the call's options, its name -- the ar member's, and
// behind "<snap_path>." the temporary's -- and what the producer's self-check counts (DEFLATE chunks, LZMA2 chunks, bzip2 blocks).
struct SnapDataMember {
    Encoder& enc;
    const char* name;
    const uint64_t& check_units;
    const double& check_ms;
};

int snap_build_impl(snaphash_ctx* x, const char* source_dir, const char* snap_path, uint32_t flags, int64_t mtime, uint8_t* archive_digest,
                    uint8_t* snap_digest, snaphash_snap_build_stats& st, const SnapDataMember& dm)
{
    const double t0 = now_ms();
    const bool hashes = !(flags & SNAPHASH_BUILD_NO_HASHES);
    SnapBuildTemps tmp;
    // the target first, as ClickDeb.Create does before Build: a target that cannot be created fails before any work
    SnapOut out;
    out.fd = open(snap_path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
    if (out.fd < 0) return fail(x, SNAPHASH_EIO, std::string(snap_path) + ": " + strerror(errno));
    host_sha512_init(out.sha);
    tmp.data = std::string(snap_path) + "." + dm.name;
    tmp.control = std::string(snap_path) + ".control.tar.gz";
    const std::string debian = go_clean(std::string(source_dir) + "/DEBIAN"); // filepath.Join(sourceDir, "DEBIAN")

    GzCheck chk_control;
    chk_control.member = "control.tar.gz";
    const bool check = (flags & SNAPHASH_BUILD_CHECK) != 0;
    uint8_t adig[64];
    char* yaml = nullptr;
    size_t yaml_len = 0;
    struct Free { char*& p; ~Free() { free(p); } } free_yaml{yaml};
    GzipEncoder enc_control(check ? &chk_control : nullptr);
    int rc = tar_create_impl(x, dm.enc, tmp.data.c_str(), source_dir, debian.c_str(), nullptr, nullptr, hashes ? &yaml : nullptr, &yaml_len, adig);
    if (rc) return rc;
    st.data_ms = x->targz.wall_ms;
    st.tar_bytes = x->targz.tar_bytes;
    st.members = x->targz.members;
    st.data_bytes = x->targz.gz_bytes;
    if (hashes) { // dataTarFinishedCallback: writeHashes' last step
        rc = write_yaml_file(x, source_dir, std::string(yaml, yaml_len));
        if (rc) return rc;
    }
    rc = tar_create_impl(x, enc_control, tmp.control.c_str(), debian.c_str(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc) return rc;
    st.control_ms = x->targz.wall_ms;
    st.control_bytes = x->targz.gz_bytes;
    st.check_chunks = dm.check_units + chk_control.chunks;
    st.check_ms = dm.check_ms + chk_control.ms;

    const double t_ar = now_ms();
    const int en = out.put((const uint8_t*)kArMagic, 8);
    if (en) return fail(x, SNAPHASH_EIO, std::string(snap_path) + ": " + strerror(en));
    rc = snap_put_member(x, out, "debian-binary", mtime, (const uint8_t*)"2.0\n", 4, nullptr);
    if (!rc) rc = snap_put_member(x, out, "_click-binary", mtime, (const uint8_t*)"0.4\n", 4, nullptr);
    if (!rc) rc = snap_put_member(x, out, "control.tar.gz", mtime, nullptr, 0, tmp.control.c_str());
    if (!rc) rc = snap_put_member(x, out, dm.name, mtime, nullptr, 0, tmp.data.c_str());
    if (rc) return rc;
    const int fd = out.fd;
    out.fd = -1;
    if (close(fd) != 0) return fail(x, SNAPHASH_EIO, std::string(snap_path) + ": " + strerror(errno));
    uint8_t sdig[64];
    host_sha512_final(out.sha, sdig);
    if (snap_digest) memcpy(snap_digest, sdig, 64);
    if (archive_digest) memcpy(archive_digest, adig, 64);
    st.snap_bytes = out.bytes;
    st.ar_ms = now_ms() - t_ar;
    st.wall_ms = now_ms() - t0;
    return SNAPHASH_OK;
}

} // namespace

extern "C" {

int snaphash_snap_build(snaphash_ctx* x, const char* source_dir, const char* snap_path, const snaphash_snap_build_options* opt,
                        uint8_t* archive_digest, uint8_t* snap_digest, snaphash_snap_build_stats* stats)
try {
    if (!x || !source_dir || !snap_path || !*snap_path) return fail(x, SNAPHASH_EINVAL, "bad argument");
    static_assert(offsetof(snaphash_snap_build_options, data_codec) == kSnapBuildOptionsSizeV1, "the codec and its options behind the 16 bytes");
    // 16: the struct before it named a codec (gzip); the whole struct and more: with data_codec, reserved, xz and bz2
    if (opt && opt->struct_size != kSnapBuildOptionsSizeV1 && opt->struct_size < sizeof(snaphash_snap_build_options))
        return fail(x, SNAPHASH_EINVAL, "snaphash_snap_build_options.struct_size");
    if (stats && stats->struct_size < sizeof(snaphash_snap_build_stats)) return fail(x, SNAPHASH_EINVAL, "snaphash_snap_build_stats.struct_size");
    const uint32_t flags = opt ? opt->flags : 0;
    if (flags & ~(uint32_t)(SNAPHASH_BUILD_NO_HASHES | SNAPHASH_BUILD_CHECK)) return fail(x, SNAPHASH_EINVAL, "unknown build flag");
    const int64_t mtime = (opt && opt->mtime >= 0) ? opt->mtime : (int64_t)time(nullptr);
    uint32_t codec = SNAPHASH_DATA_GZ;
    const snaphash_xz_options* xo = nullptr;
    const snaphash_bz2_options* bo = nullptr;
    if (opt && opt->struct_size >= sizeof(snaphash_snap_build_options)) {
        codec = opt->data_codec;
        xo = opt->xz;
        bo = opt->bz2;
        if (codec > SNAPHASH_DATA_XZ) return fail(x, SNAPHASH_EINVAL, "snap build: data_codec is 0 (gz), 1 (bz2) or 2 (xz)");
        if (opt->reserved) return fail(x, SNAPHASH_EINVAL, "snap build: snaphash_snap_build_options.reserved is not 0");
        if ((xo && codec != SNAPHASH_DATA_XZ) || (bo && codec != SNAPHASH_DATA_BZ2))
            return fail(x, SNAPHASH_EINVAL, "snap build: options for a codec that is not data_codec");
    }
    const bool check = (flags & SNAPHASH_BUILD_CHECK) != 0;
    snaphash_snap_build_stats st{};
    st.struct_size = sizeof st;
    auto build = [&](const SnapDataMember& dm) {
        const int rc = snap_build_impl(x, source_dir, snap_path, flags, mtime, archive_digest, snap_digest, st, dm);
        if (rc) (void)unlink(snap_path);
        if (stats) *stats = st;
        return rc;
    };
    // the data member's encoder is this call's own, made with this call's options: nothing of it outlives the call
    if (codec == SNAPHASH_DATA_XZ) {
        uint64_t bs;
        uint32_t chk, level;
        XzEncChain filter;
        bool self;
        int rc = xz_read_options(x, xo, &bs, &chk, &self, &filter, &level);
        if (rc) return rc;
        XzSelfCheck sc;
        sc.member = "data.tar.xz";
        XzEncoder enc(bs, chk, (self || check) ? &sc : nullptr, filter, level);
        rc = build(SnapDataMember{enc, "data.tar.xz", sc.chunks, sc.ms});
        xz_keep_selfcheck_stats(x, sc);
        xz_keep_filter_stats(x, enc);
        return rc;
    }
    if (codec == SNAPHASH_DATA_BZ2) {
        uint32_t level;
        bool self;
        int rc = bz2_read_options(x, bo, &level, &self);
        if (rc) return rc;
        BzSelfCheck sc;
        sc.member = "data.tar.bz2";
        BzEncoder enc(level, (self || check) ? &sc : nullptr);
        rc = build(SnapDataMember{enc, "data.tar.bz2", sc.blocks, sc.ms});
        bz2_keep_selfcheck_stats(x, sc);
        return rc;
    }
    GzCheck chk_data;
    chk_data.member = "data.tar.gz";
    GzipEncoder enc(check ? &chk_data : nullptr);
    return build(SnapDataMember{enc, "data.tar.gz", chk_data.chunks, chk_data.ms});
} catch (...) { // allocation or thread-creation failure: no C++ exception crosses the C boundary
    if (snap_path) (void)unlink(snap_path);
    return SNAPHASH_ENOMEM;
}

int snaphash_deflate_check_device(snaphash_ctx* x, const void* d_in, size_t n_in, const void* d_z, const uint64_t* z_off, size_t nchunks,
                                  int last_is_final, snaphash_deflate_verdict* verdicts)
try {
    static_assert(sizeof(snaphash_deflate_verdict) == sizeof(DfCheckVerdict), "the verdicts travel as they are");
    if (!x || !z_off || !verdicts || nchunks == 0 || nchunks > 0x7fffffffu || (n_in && !d_in) || (uint64_t)nchunks * kDfCheckChunk < n_in)
        return fail(x, SNAPHASH_EINVAL, "bad argument");
    for (size_t i = 0; i < nchunks; ++i)
        if (z_off[i] > z_off[i + 1]) return fail(x, SNAPHASH_EINVAL, "z_off descends");
    if (z_off[nchunks] && !d_z) return fail(x, SNAPHASH_EINVAL, "bad argument");
    TOP_ENTER(x);
    DevCtx* c = x->d0();
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<uint64_t> d_off;
    DevBuf<DfCheckVerdict> d_v;
    HIP_TRY(c, d_off.reserve(nchunks + 1));
    HIP_TRY(c, d_v.reserve(nchunks));
    HIP_TRY(c, hipMemcpyAsync(d_off.data(), z_off, (nchunks + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(d_v.data(), 0xff, nchunks * sizeof(DfCheckVerdict), c->stream));
    HIP_TRY(c, launch_deflate_check((const uint8_t*)d_in, n_in, (const uint8_t*)d_z, z_off[nchunks], d_off.data(), nullptr, 0, (uint32_t)nchunks,
                                    (uint32_t)nchunks, last_is_final != 0, d_v.data(), c->stream));
    HIP_TRY(c, hipMemcpyAsync(verdicts, d_v.data(), nchunks * sizeof(DfCheckVerdict), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    x->stats.launches = 1;
    end_top(x, t_top0_);
    return SNAPHASH_OK;
} catch (...) { // allocation failure: no C++ exception crosses the C boundary
    return SNAPHASH_ENOMEM;
}

} // extern "C"
