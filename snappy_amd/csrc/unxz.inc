// unxz.inc -- the data.tar.xz side of the install path, textually part of snaphash_api.cpp (after unpack.inc, which
// owns DecodedStream and everything behind the decoder; this file owns the .xz decoder and its codec entry, kUnxzCodec).
//
// The reference's ClickDeb.Unpack takes data.tar.{gz,bz2,xz} (clickdeb/deb.go:185); skipToArMember (deb.go:408-441)
// pipes the .xz member through the xz program.  Here the file's Index says where every Block begins and where its bytes
// go (xz_core.h xz_plan), so the Blocks are decoded side by side, each straight to its final offset -- on host threads
// in the default configuration (xz_host.cpp), by lzma2_blocks_kernel (xz_kernels.hip) under SNAPHASH_FLAG_GPU_ONLY, where
// the CRC-32, CRC-64 and SHA-256 Checks are taken in HBM right after the decode (crc_kernels.hip, sha256_kernels.hip) -- and
// the decoded stream goes through the same unpack and in-pass Verify as data.tar.gz.  The _ex entries' SNAPHASH_UNXZ_BCJ
// also takes Blocks with an x86, ARM or ARM-Thumb filter in front of LZMA2 (DESIGN.md sec. 25): the filter is undone behind
// the Block's decode and in front of its Check, by the Block's host thread or by bcj_kernels.hip over what the kernel decoded.
// SNAPHASH_UNXZ_CHAINS takes every chain liblzma 5.2.5 reads (sec. 29): up to three of Delta and the six BCJ filters, undone
// the same way, a stage of the filter kernels a place in the chain.

namespace {

// Decodes every Stream of xz[0..n) and appends the bytes to ds.out; keep_dev: the whole decoded stream also stays in
// c->inf.d_out[0..out.size()) for Verify's device hashing, as gunzip_engine leaves it.  Where a codec's decoder is told to
// take its CRCs is not read: under SNAPHASH_FLAG_GPU_ONLY the Checks are taken in HBM whoever calls, on host threads
// otherwise.  tally (may be null; the .snap session's): the Blocks' Checks of this decode are added to it on every way out,
// a range a Block, from what snaphash_get_xz_check_stats hands out.
int unxz_engine(snaphash_ctx* x, DevCtx* c, const uint8_t* xz, size_t n, DecodedStream& ds, snaphash_unpack_stats& st, CrcAt, CrcTally* tally)
{
    struct TallyChecks {
        CrcTally* const t;
        const snaphash_xz_check_stats& ck;
        bool armed = false; // once ck is this decode's
        ~TallyChecks()
        {
            if (!t || !armed) return;
            t->device_ranges += ck.device_crc32 + ck.device_crc64 + ck.device_sha256;
            t->host_ranges += ck.host_checks;
            t->device_ms += ck.device_check_ms;
        }
    } tally_checks{tally, x->xz_check};

    std::vector<uint8_t>& out = ds.out;
    std::vector<XzBlock> blocks;
    uint64_t total = 0;
    std::string why;
    x->xz_filter = snaphash_xz_filter_stats{};
    const int pe = xz_plan(xz, n, blocks, &total, why, x->unxz_chains ? kXzChainAny : x->unxz_bcj ? kXzChainBcj : kXzChainNone); // (the _ex entries' flags)
    if (pe) return fail(c, pe == kXzPlanUnsupported ? SNAPHASH_EINVAL : SNAPHASH_EFORMAT, why);
    c->fout_gen++;
    snaphash_xz_filter_stats& fs = x->xz_filter; // who undid the Blocks' filters
    auto host_filtered = [&](const std::vector<uint32_t>* which) {
        const size_t K = which ? which->size() : blocks.size();
        for (size_t k = 0; k < K; ++k) {
            const XzBlock& b = blocks[which ? (*which)[k] : k];
            if (b.nfilt) { fs.host_blocks++; fs.filter = b.filt[0]; } // (a Block counts once, by the filter its header names first)
        }
    };
    snaphash_xz_check_stats& ck = x->xz_check; // who took the Checks of this decode
    ck = snaphash_xz_check_stats{};
    ck.struct_size = sizeof ck;
    tally_checks.armed = true;
    auto host_checked = [&](const std::vector<uint32_t>* which) {
        const size_t K = which ? which->size() : blocks.size();
        for (size_t k = 0; k < K; ++k) ck.host_checks += blocks[which ? (*which)[k] : k].check != kXzCheckNone;
    };
    const unsigned cpus = call_cpus(x);
    const size_t o0 = out.size();
    out.resize(o0 + total);
    uint8_t* dst = out.data() + o0;
    const uint64_t base = ds.dev_base(o0); // where the result begins in c->inf.d_out
    int rc = DecodedStream::stream(c);
    if (rc) return rc;
    st.segments += blocks.size();
    if (!x->gpu_only) {
        // the default configuration: a Block a host thread (DESIGN.md sec. 17)
        if (xz_blocks_host(xz, blocks, nullptr, dst, cpus)) {
            ds.rollback();
            return fail(c, SNAPHASH_EFORMAT, "xz: corrupt block");
        }
        st.host_bytes += total;
        host_checked(nullptr);
        host_filtered(nullptr);
        return ds.mirror(o0, o0 + total);
    }
    // SNAPHASH_FLAG_GPU_ONLY: every Block up to kXzGpuBlockMax through the kernel, the rest (and what the kernel refuses) on
    // host threads
    std::vector<uint32_t> gpu, host;
    for (uint32_t i = 0; i < blocks.size(); ++i) (blocks[i].out_len <= kXzGpuBlockMax ? gpu : host).push_back(i);
    rc = ds.reserve_dev(c, std::max<uint64_t>(base + total, 1), base);
    if (rc) return rc;
    if (!gpu.empty()) {
        float kms = 0;
        double cms = 0;
        HIP_TRY(c, c->xz.ensure(n, gpu.size()));
        HIP_TRY(c, hipMemcpyAsync(c->xz.d_in.data(), xz, n, hipMemcpyHostToDevice, c->f_stream));
        for (size_t k = 0; k < gpu.size(); ++k) {
            const XzBlock& b = blocks[gpu[k]];
            c->xz.blk.h[k] = XzGpuBlock{b.in_off, b.in_len, base + b.out_off, b.out_len, b.dict_size, (uint32_t)kXzBad};
        }
        HIP_TRY(c, hipMemcpyAsync(c->xz.blk.d.data(), c->xz.blk.h.data(), gpu.size() * sizeof(XzGpuBlock), hipMemcpyHostToDevice, c->f_stream));
        Span ev;
        if ((rc = span_begin(c, Ev::Codec, c->f_stream, &ev))) return rc;
        HIP_TRY(c, launch_lzma2_blocks(c->xz.d_in.data(), c->inf.d_out.data(), c->xz.blk.d.data(), (uint32_t)gpu.size(), c->f_stream));
        if ((rc = span_end(c, ev, c->f_stream))) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->xz.blk.h.data(), c->xz.blk.d.data(), gpu.size() * sizeof(XzGpuBlock), hipMemcpyDeviceToHost, c->f_stream));
        HIP_TRY(c, hipStreamSynchronize(c->f_stream));
        kms = span_ms(ev);
        st.inflate_ms += kms;
        scratch_spans_done(c);
        // the Checks of what the kernel decoded, in HBM, a range a Block
        std::vector<uint32_t> ok, k32, k64, k256;
        for (size_t k = 0; k < gpu.size(); ++k) {
            if (c->xz.blk.h[k].status != kXzOk) { host.push_back(gpu[k]); continue; } // the host decoder says what is wrong
            ok.push_back(gpu[k]);
            if (blocks[gpu[k]].check == kXzCheckCrc32) k32.push_back(gpu[k]);
            if (blocks[gpu[k]].check == kXzCheckCrc64) k64.push_back(gpu[k]);
            if (blocks[gpu[k]].check == kXzCheckSha256) k256.push_back(gpu[k]);
        }
        // the filters of what the kernel decoded, undone in HBM, a range a Block: in front of the Checks, which are over the
        // unfiltered bytes, and of the copies back.  A chain of k filters is k stages over the table (sec. 29), the filter
        // nearest LZMA2 first; a Block whose chain is shorter has no filter at the later stages and is skipped there
        uint32_t stages = 0;
        size_t filtered = 0;
        for (uint32_t i : ok) {
            stages = std::max(stages, blocks[i].nfilt);
            if (blocks[i].nfilt) { filtered++; fs.filter = blocks[i].filt[0]; }
        }
        if (stages) {
            if (c->bcj_ev[0].ensure() != hipSuccess || c->bcj_ev[1].ensure() != hipSuccess) return fail(c, SNAPHASH_EDEVICE, "hipEventCreate failed");
            HIP_TRY(c, hipEventRecord(c->bcj_ev[0], c->f_stream));
            std::vector<BcjRange> fr;
            for (uint32_t j = 0; j < stages; ++j) {
                fr.clear();
                for (uint32_t i : ok) {
                    const XzBlock& b = blocks[i];
                    if (!b.nfilt) continue;
                    const bool has = b.nfilt > j;
                    fr.push_back(BcjRange{base + b.out_off, b.out_len, 0, has ? b.filt[b.nfilt - 1 - j] : 0u, has ? b.fparam[b.nfilt - 1 - j] : 0u, 0});
                }
                rc = xz_filter_stage_dev(c, c->inf.d_out.data(), fr, false, c->f_stream, nullptr, nullptr);
                if (rc) return rc;
            }
            HIP_TRY(c, hipEventRecord(c->bcj_ev[1], c->f_stream));
            fs.device_blocks = filtered;
        }
        // the bytes of the Blocks the kernel decoded on their way back (neighbours in one copy), beside the Check kernels;
        // what a host thread will decode is not moved
        for (size_t k = 0; k < ok.size();) {
            const uint64_t from = blocks[ok[k]].out_off;
            uint64_t to = from + blocks[ok[k]].out_len;
            for (++k; k < ok.size() && blocks[ok[k]].out_off == to; ++k) to += blocks[ok[k]].out_len;
            rc = ds.fetch(o0, o0 + from, o0 + to);
            if (rc) return rc;
        }
        std::vector<uint64_t> offs, lens;
        auto ranges = [&](const std::vector<uint32_t>& v) {
            offs.resize(v.size());
            lens.resize(v.size());
            for (size_t k = 0; k < v.size(); ++k) { offs[k] = base + blocks[v[k]].out_off; lens[k] = blocks[v[k]].out_len; }
        };
        bool bad = false;
        if (!k32.empty()) {
            ranges(k32);
            std::vector<uint32_t> got(k32.size());
            rc = crc_ranges_dev(c, kCrcGzip, c->inf.d_out.data(), offs.data(), lens.data(), k32.size(), got.data(), c->f_stream, &cms);
            scratch_spans_done(c);
            if (rc) return rc;
            for (size_t k = 0; k < k32.size(); ++k) bad |= got[k] != xz_le32(xz + blocks[k32[k]].check_off);
        }
        if (!k64.empty()) {
            ranges(k64);
            std::vector<uint64_t> got(k64.size());
            rc = crc_ranges_dev(c, 0, c->inf.d_out.data(), offs.data(), lens.data(), k64.size(), got.data(), c->f_stream, &cms);
            scratch_spans_done(c);
            if (rc) return rc;
            for (size_t k = 0; k < k64.size(); ++k) {
                const uint8_t* f = xz + blocks[k64[k]].check_off;
                bad |= got[k] != ((uint64_t)xz_le32(f + 4) << 32 | xz_le32(f));
            }
        }
        if (!k256.empty()) {
            ranges(k256);
            std::vector<uint8_t> got(k256.size() * kSha256Digest);
            rc = sha256_ranges_dev(c, c->inf.d_out.data(), offs.data(), lens.data(), k256.size(), got.data(), c->f_stream, &cms);
            scratch_spans_done(c);
            if (rc) return rc;
            for (size_t k = 0; k < k256.size(); ++k) bad |= memcmp(got.data() + k * kSha256Digest, xz + blocks[k256[k]].check_off, kSha256Digest) != 0;
        }
        HIP_TRY(c, hipStreamSynchronize(c->f_stream)); // (the bytes are back: the Check calls waited on the same stream, but there may be none)
        st.inflate_ms += cms;
        if (stages) {
            const float fms = span_ms(Span{c->bcj_ev[0], c->bcj_ev[1]});
            fs.device_ms = fms;
            st.inflate_ms += fms;
        }
        ck.device_crc32 = k32.size();
        ck.device_crc64 = k64.size();
        ck.device_sha256 = k256.size();
        ck.device_check_ms = cms;
        if (bad) {
            ds.rollback();
            return fail(c, SNAPHASH_EFORMAT, "xz: block check mismatch");
        }
        st.gpu_segments += ok.size();
    }
    if (!host.empty()) {
        if (xz_blocks_host(xz, blocks, &host, dst, cpus)) {
            ds.rollback();
            return fail(c, SNAPHASH_EFORMAT, "xz: corrupt block");
        }
        host_checked(&host);
        host_filtered(&host);
        for (uint32_t i : host) {
            st.host_bytes += blocks[i].out_len;
            rc = ds.mirror_async(o0 + blocks[i].out_off, o0 + blocks[i].out_off + blocks[i].out_len);
            if (rc) return rc;
        }
        rc = ds.sync();
        if (rc) return rc;
    }
    return SNAPHASH_OK;
}

const UnpackCodec kUnxzCodec = {"xz", unxz_engine};

// What an _ex entry was asked for, for the length of its call: unxz_engine reads x->unxz_bcj (a codec's decoder takes no
// options of its own).  opt == nullptr or all zero: the plain entries' behaviour.
struct UnxzCall {
    snaphash_ctx* const x;
    explicit UnxzCall(snaphash_ctx* x_) : x(x_) {}
    ~UnxzCall() { x->unxz_bcj = x->unxz_chains = false; }
    void allow_bcj() { x->unxz_bcj = true; } // (a .snap session opened with SNAPHASH_SNAP_XZ, snap.inc)
    void allow_chains() { x->unxz_chains = true; } // (and with SNAPHASH_SNAP_XZ_CHAINS)
    int read(const snaphash_unxz_options* opt)
    {
        if (!opt || (opt->struct_size == 0 && opt->flags == 0)) return SNAPHASH_OK;
        if (opt->struct_size < sizeof(snaphash_unxz_options)) return fail(x, SNAPHASH_EINVAL, "snaphash_unxz_options.struct_size");
        if (opt->flags & ~(uint32_t)(SNAPHASH_UNXZ_BCJ | SNAPHASH_UNXZ_CHAINS)) return fail(x, SNAPHASH_EINVAL, "xz: unknown flag");
        x->unxz_bcj = (opt->flags & SNAPHASH_UNXZ_BCJ) != 0;
        x->unxz_chains = (opt->flags & SNAPHASH_UNXZ_CHAINS) != 0;
        return SNAPHASH_OK;
    }
};

} // namespace

extern "C" {

int snaphash_unxz_buffer(snaphash_ctx* x, const void* xz, size_t n, void** out, size_t* out_len)
{
    return decode_to_malloc(x, kUnxzCodec, xz, n, out, out_len);
}

int snaphash_tar_unpack_xz(snaphash_ctx* x, const char* data_tar_xz, const char* target_dir, const char* yaml, size_t yaml_len,
                           snaphash_mismatch* first, uint8_t* archive_digest)
{
    return tar_unpack_entry(x, kUnxzCodec, data_tar_xz, target_dir, yaml, yaml_len, first, archive_digest);
}

int snaphash_unxz_buffer_ex(snaphash_ctx* x, const void* xz, size_t n, const snaphash_unxz_options* opt, void** out, size_t* out_len)
{
    if (!x) return SNAPHASH_EINVAL;
    UnxzCall call(x);
    if (int rc = call.read(opt)) return rc;
    return decode_to_malloc(x, kUnxzCodec, xz, n, out, out_len);
}

int snaphash_tar_unpack_xz_ex(snaphash_ctx* x, const char* data_tar_xz, const char* target_dir, const char* yaml, size_t yaml_len,
                              const snaphash_unxz_options* opt, snaphash_mismatch* first, uint8_t* archive_digest)
{
    if (!x) return SNAPHASH_EINVAL;
    UnxzCall call(x);
    if (int rc = call.read(opt)) return rc;
    return tar_unpack_entry(x, kUnxzCodec, data_tar_xz, target_dir, yaml, yaml_len, first, archive_digest);
}

int snaphash_get_xz_filter_stats(const snaphash_ctx* x, snaphash_xz_filter_stats* out)
{
    if (!x || !out || out->struct_size < sizeof(snaphash_xz_filter_stats)) return SNAPHASH_EINVAL;
    *out = x->xz_filter;
    out->struct_size = sizeof(snaphash_xz_filter_stats);
    return SNAPHASH_OK;
}

int snaphash_get_xz_check_stats(const snaphash_ctx* x, snaphash_xz_check_stats* out)
{
    if (!x || !out) return SNAPHASH_EINVAL;
    *out = x->xz_check;
    out->struct_size = sizeof *out;
    return SNAPHASH_OK;
}

int snaphash_unxz_block_device(snaphash_ctx* x, const void* xz, size_t n, size_t block, void* d_dst, size_t dst_len)
try {
    if (!x || !xz || !d_dst) return fail(x, SNAPHASH_EINVAL, "bad argument");
    TOP_ENTER(x);
    DevCtx* c = x->d0();
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<XzBlock> blocks;
    uint64_t total = 0;
    std::string why;
    const int pe = xz_plan((const uint8_t*)xz, n, blocks, &total, why);
    if (pe) return fail(x, pe == kXzPlanUnsupported ? SNAPHASH_EINVAL : SNAPHASH_EFORMAT, why);
    if (block >= blocks.size() || blocks[block].out_len != dst_len) return fail(x, SNAPHASH_EINVAL, "xz: no such Block, or dst_len is not its uncompressed size");
    const XzBlock& b = blocks[block];
    if (b.out_len > kXzGpuBlockMax) return fail(x, SNAPHASH_EINVAL, "xz: the Block is larger than the kernel takes");
    if (int rc = DecodedStream::stream(c)) return lift(x, c, rc);
    HIP_TRY(c, c->xz.ensure(b.in_len, 1));
    HIP_TRY(c, hipMemcpyAsync(c->xz.d_in.data(), (const uint8_t*)xz + b.in_off, b.in_len, hipMemcpyHostToDevice, c->f_stream));
    c->xz.blk.h[0] = XzGpuBlock{0, b.in_len, 0, b.out_len, b.dict_size, (uint32_t)kXzBad};
    HIP_TRY(c, hipMemcpyAsync(c->xz.blk.d.data(), c->xz.blk.h.data(), sizeof(XzGpuBlock), hipMemcpyHostToDevice, c->f_stream));
    HIP_TRY(c, launch_lzma2_blocks(c->xz.d_in.data(), (uint8_t*)d_dst, c->xz.blk.d.data(), 1, c->f_stream));
    HIP_TRY(c, hipMemcpyAsync(c->xz.blk.h.data(), c->xz.blk.d.data(), sizeof(XzGpuBlock), hipMemcpyDeviceToHost, c->f_stream));
    HIP_TRY(c, hipStreamSynchronize(c->f_stream));
    end_top(x, t_top0_);
    if (c->xz.blk.h[0].status != kXzOk) return fail(x, SNAPHASH_EFORMAT, "xz: corrupt block");
    return SNAPHASH_OK;
} catch (...) { // allocation failure: no C++ exception crosses the C boundary
    return SNAPHASH_ENOMEM;
}

} // extern "C"
