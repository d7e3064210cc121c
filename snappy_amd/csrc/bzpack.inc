// bzpack.inc -- the data.tar.bz2 producer, textually part of snaphash_api.cpp (behind targz.inc, whose pass, consumers,
// staging and buffer driver it shares: BzEncoder is one of targz.inc's Encoders, as xzpack.inc's XzEncoder is).
//
// The reference's tarCreate refuses a ".bz2" name (clickdeb/deb.go:274-275) and snaphash_tar_create keeps doing so; this
// is the writer of the one format the install side reads (ClickDeb.Unpack, deb.go:185) and the library could not write.
// The staged tar stream is cut into pieces of bzenc_piece(level) bytes, a bzip2 block each (bzip2_enc_core.h), and a
// staging slot is a whole number of pieces, no more than one launch codes: the blocks' CRCs come from crc_kernels.hip over
// the staged bytes, bzip2_enc_kernels.hip runs RLE1, the BWT, MTF and the Huffman coding of every block of the slot side by
// side and shifts their bits together.  The host adds the four bytes in front and the footer, folds the combined CRC, and
// holds the stream's last partial byte back until the next slot (or the footer) completes it.  Asked to
// (SNAPHASH_BZ2_SELF_CHECK), it has every block of a slot decoded again in HBM by the install side's kernels and compared
// with the staged piece before the bytes go on (bz2_check_core.h, bz2_check_kernels.hip; DESIGN.md sec. 24).

namespace {

// blocks of one launch: their BWT scratch together stays under kBzEncLaunchBytes x kBzEncScratchPerByte (0.8 GB)
uint32_t bz_launch_blocks(uint32_t level) { return (uint32_t)std::min<uint64_t>(kBzEncLaunchBlocksMax, kBzEncLaunchBytes / bzenc_rle_cap(level)); }

// the producer's slot: whole pieces, as many as the job has, the staging size holds and one launch takes (at least one)
uint64_t bz_slot_bytes(const DevCtx* c, uint64_t job_bytes, uint32_t level)
{
    const uint64_t P = bzenc_piece(level);
    const uint64_t want = std::max<uint64_t>(1, (job_bytes + P - 1) / P);
    return std::max<uint64_t>(1, std::min({want, c->staging / P, (uint64_t)bz_launch_blocks(level)})) * P;
}

// with_output: the producer's; without: the scratch of the stages alone (snaphash_bwt_device)
int ensure_bzenc(DevCtx* c, uint32_t blocks, uint32_t cap, bool with_output)
{
    const int rc = ensure_producer_streams(c);
    if (rc) return rc;
    HIP_TRY(c, c->be.ensure(blocks, cap, with_output, c->numa_node)); // (a failure leaves none of it)
    return SNAPHASH_OK;
}

// The .bz2 producer's self-check (DESIGN.md sec. 24), asked for by the _ex entries' SNAPHASH_BZ2_SELF_CHECK alone: every slot's
// blocks are decoded again in HBM and compared with the staged pieces before they leave it (bz2_check_core.h).
struct BzSelfCheck {
    const char* member = ""; // for last_error
    uint64_t blocks = 0;     // blocks checked (all accepted, or the call failed)
    double ms = 0;           // the check's kernels, HIP events
    uint64_t bytes = 0;      // of the tar stream, in the slots checked so far
};

// The check's groups are the install side's batches (unbz2.inc's kBzLaunchSlots, which asserts the two agree): 256 slots of
// Bzip2Bufs at most, 4.5 MB each.
constexpr uint32_t kBz2CheckGroup = 256;

// The four steps of the check over `count` blocks, enqueued on s and not waited for (but under stage_ms, which waits for every
// group to time its steps): table entries d_jobs and verdicts d_verdicts in HBM, the compressed bytes d_z[0 .. n_z), the
// staged stream d_in[0 .. n_in).  The scratch is the install side's, c->bz, through its own ensure, a group of at most
// kBz2CheckGroup blocks at a time; c->inf.d_out is not touched.  stage_ms: symbols, link, inverse BWT + RLE1 count, compare.
int bz2_check_run(DevCtx* c, const uint8_t* d_z, uint64_t n_z, const uint8_t* d_in, uint64_t n_in, const Bz2CheckJob* d_jobs, uint32_t count,
                  uint32_t level, Bz2Verdict* d_verdicts, hipStream_t s, float* stage_ms)
{
    if (count == 0) return SNAPHASH_OK;
    HIP_TRY(c, c->bz.ensure(0, std::min(count, kBz2CheckGroup), c->numa_node));
    Bzip2Bufs& z = c->bz;
    StageClock<4> clk; // (off without stage_ms: its marks do nothing then)
    if (stage_ms) HIP_TRY(c, clk.enable());
    for (uint32_t g0 = 0; g0 < count; g0 += kBz2CheckGroup) {
        const uint32_t nb = std::min(kBz2CheckGroup, count - g0);
        if (nb > z.nslots()) return fail(c, SNAPHASH_EDEVICE, "bzip2: the self-check's scratch is smaller than its group");
        HIP_TRY(c, clk.mark(0, s));
        HIP_TRY(c, launch_bz2_check_symbols(d_z, n_z, n_in, d_jobs + g0, level, nb, z.d_slots.data(), z.d_res.data(), s));
        HIP_TRY(c, clk.mark(1, s));
        HIP_TRY(c, launch_bz2_check_link(z.d_res.data(), d_jobs + g0, n_z, n_in, level, nb, z.d_blk.data(), d_verdicts + g0, s));
        HIP_TRY(c, clk.mark(2, s));
        HIP_TRY(c, launch_bz_ibwt(z.d_slots.data(), z.d_tt.data(), z.d_blk.data(), nb, s));
        HIP_TRY(c, launch_bz_rle1_count(z.d_slots.data(), z.d_blk.data(), z.d_chunks.data(), nb, s));
        HIP_TRY(c, clk.mark(3, s));
        HIP_TRY(c, launch_bz2_check_compare(z.d_slots.data(), z.d_blk.data(), z.d_chunks.data(), d_in, d_jobs + g0, nb, d_verdicts + g0, s));
        if (stage_ms) {
            HIP_TRY(c, clk.mark(4, s));
            HIP_TRY(c, hipStreamSynchronize(s));
            for (int i = 0; i < 4; ++i) stage_ms[i] += clk.ms(i);
        }
    }
    return SNAPHASH_OK;
}

// The .bz2 encoder of one call: the level it was asked for (1 to 9), the combined CRC so far, and the stream's last, partial
// byte -- held back until the next slot's blocks (or the footer) complete it.
struct BzEncoder final : Encoder {
    const uint32_t level;
    uint32_t crc = 0, carry = 0, carry_bits = 0;
    BzSelfCheck* const self_check; // null = off, the producer's path without it
    explicit BzEncoder(uint32_t lvl = 9, BzSelfCheck* sc = nullptr)
        : Encoder(".bz2", "bzip2: a block's input is larger than the engine's staging size"), level(lvl), self_check(sc)
    {
        if (sc) check_ms = &sc->ms;
    }
    uint64_t slot_bytes(const DevCtx* c, uint64_t job_bytes) const override { return bz_slot_bytes(c, job_bytes, level); }
    int ensure(DevCtx* c, uint64_t slot_bytes) override
    {
        const uint32_t blocks = (uint32_t)(slot_bytes / bzenc_piece(level));
        const int rc = ensure_bzenc(c, blocks, bzenc_rle_cap(level), true);
        if (rc || !self_check) return rc;
        HIP_TRY(c, c->be.ensure_check(c->be.made_blocks));
        HIP_TRY(c, c->bz.ensure(0, std::min(blocks, kBz2CheckGroup), c->numa_node));
        return SNAPHASH_OK;
    }
    void begin(OutPipe& g) override
    {
        const uint8_t h[kBzEncStreamHead] = {'B', 'Z', 'h', (uint8_t)('0' + level)};
        gz_emit(g, h, sizeof h, -1);
    }
    int slot(OutPipe& g, Slot& sl, uint64_t n, hipEvent_t ready, int zbuf, bool is_first, bool is_last) override;
    int finish(OutPipe& g, uint8_t archive_digest[64]) override // the end-of-stream magic and the combined CRC behind the held-back bits
    {
        uint32_t tail[4] = {carry & 0xffu, 0, 0, 0}; // (memory in stream order: the held-back byte is byte 0)
        BzW w;
        bzw_start(w, tail, 4, carry_bits);
        bzw_put(w, (uint32_t)(kBzEosMagic >> 24), 24);
        bzw_put(w, (uint32_t)(kBzEosMagic & 0xffffffu), 24);
        bzw_put(w, crc, 32);
        const uint64_t bytes = (bzw_pos(w) + 7) / 8;
        bzw_flush(w);
        return pipe_finish(g, (const uint8_t*)tail, (size_t)bytes, archive_digest);
    }
};

// The self-check of a slot, behind bz_enc_concat_kernel on the compressor's stream: the nblk blocks' bit stretches of
// b.d_out[0 .. out_words) against their pieces of the slot's staged bytes.  A stretch begins where the host placed the block
// (b.dst; the first one at carry_bits: the held-back byte is in the buffer) and ends where the next one begins, or at the
// slot's `at` -- not where the block's own end-of-block symbol says; pieces and CRCs are the host's own.  Waits for the
// verdicts; a refused block fails the call.
int bz_self_check_slot(OutPipe& g, BzEncoder& z, Slot& sl, uint64_t n, uint32_t nblk, uint64_t at, uint64_t out_words,
                       const std::vector<uint64_t>& offs, const std::vector<uint64_t>& lens, const std::vector<uint32_t>& crcs, bool trace)
{
    DevCtx* c = g.c;
    BzEncBufs& b = c->be;
    hipStream_t zs = c->z_stream;
    BzSelfCheck& sc = *z.self_check;
    if (b.ckjobs.size() < nblk || b.chk.size() < nblk) return fail(c, SNAPHASH_EDEVICE, "bzip2: the self-check's tables are smaller than the slot");
    for (uint32_t k = 0; k < nblk; ++k) b.ckjobs.h[k] = Bz2CheckJob{b.dst.h[k], k + 1 < nblk ? b.dst.h[k + 1] : at, offs[k], lens[k], crcs[k], 0};
    HIP_TRY(c, hipMemcpyAsync(b.ckjobs.d.data(), b.ckjobs.h.data(), (size_t)nblk * sizeof(Bz2CheckJob), hipMemcpyHostToDevice, zs));
    HIP_TRY(c, hipMemsetAsync(b.chk.d.data(), 0xff, (size_t)nblk * sizeof(Bz2Verdict), zs)); // (a verdict that is not written is a refusal)
    float stage_ms[4] = {0, 0, 0, 0};
    Span ev;
    int rc = span_begin(c, Ev::Check, zs, &ev);
    if (!rc) rc = bz2_check_run(c, (const uint8_t*)b.d_out.data(), out_words * 4, sl.d_buf.data(), n, b.ckjobs.d.data(), nblk, z.level, b.chk.d.data(),
                                 zs, trace ? stage_ms : nullptr);
    if (!rc) rc = span_end(c, ev, zs);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(b.chk.h.data(), b.chk.d.data(), (size_t)nblk * sizeof(Bz2Verdict), hipMemcpyDeviceToHost, zs));
    HIP_TRY(c, hipStreamSynchronize(zs));
    if (trace)
        fprintf(stderr, "snaphash bz2 self-check: %u blocks: symbols %.3f ms, link %.3f ms, ibwt+rle1 %.3f ms, compare %.3f ms\n", nblk, stage_ms[0],
                stage_ms[1], stage_ms[2], stage_ms[3]);
    for (uint32_t k = 0; k < nblk; ++k) {
        const Bz2Verdict v = b.chk.h[k];
        if (v.status == kBz2CheckOk) continue;
        // (the block counts through the whole stream: bz_process_slot calls this BEFORE it adds the slot's blocks to
        // g.st.chunks, and sc.bytes grows below; the offset is the differing byte for status 1 and 2, else the piece's first)
        const uint64_t in_piece = v.status == kBz2CheckByte || v.status == kBz2CheckLength ? v.offset : 0;
        return fail(c, SNAPHASH_EDEVICE, bz2_check_error_text(sc.member, g.st.chunks + k, v.status, sc.bytes + offs[k] + in_piece));
    }
    sc.blocks += nblk;
    sc.bytes += n;
    return SNAPHASH_OK;
}

// The slot's first n bytes (in sl.d_buf once `ready` has fired; nullptr: already ordered on the compressor's stream) as
// blocks into c->be.h_out[zbuf] and on to the consumers.
int bz_process_slot(OutPipe& g, BzEncoder& z, Slot& sl, uint64_t n, hipEvent_t ready, int zbuf, bool, bool)
{
    if (n == 0) return SNAPHASH_OK;
    DevCtx* c = g.c;
    BzEncBufs& b = c->be;
    hipStream_t zs = c->z_stream;
    const uint64_t P = bzenc_piece(z.level);
    const uint32_t nblk = (uint32_t)((n + P - 1) / P);
    if (n > sl.cap() || nblk > b.made_blocks || bzenc_rle_cap(z.level) > b.made_cap || !b.h_out[0].size())
        return fail(c, SNAPHASH_EDEVICE, "bzip2: the encoder's buffers are smaller than the slot");
    if (ready) HIP_TRY(c, hipStreamWaitEvent(zs, ready, 0));
    // the blocks' CRCs: over the pieces as they are, before RLE1
    std::vector<uint64_t> offs(nblk), lens(nblk);
    std::vector<uint32_t> crcs(nblk);
    for (uint32_t k = 0; k < nblk; ++k) {
        offs[k] = (uint64_t)k * P;
        lens[k] = std::min<uint64_t>(P, n - offs[k]);
    }
    double crc_ms = 0;
    int rc = crc_ranges_dev(c, kCrcBzip2, sl.d_buf.data(), offs.data(), lens.data(), nblk, crcs.data(), zs, &crc_ms);
    if (rc) return rc;
    for (uint32_t k = 0; k < nblk; ++k) b.jobs.h[k] = BzEncJob{offs[k], (uint32_t)lens[k], crcs[k]};
    const BzEncScratch s = b.scratch();
    HIP_TRY(c, hipMemcpyAsync(b.jobs.d.data(), b.jobs.h.data(), (size_t)nblk * sizeof(BzEncJob), hipMemcpyHostToDevice, zs));
    const bool trace = getenv("SNAPHASH_TRACE_BZ2") != nullptr; // the stages one by one (tools/bzip2_enc_bench.py reads the line)
    StageClock<4> stages; // (launch_bzenc_blocks records them itself, between its kernels)
    if (trace) HIP_TRY(c, stages.enable());
    Span ev, ev2;
    if ((rc = span_begin(c, Ev::Codec, zs, &ev))) return rc;
    HIP_TRY(c, launch_bzenc_blocks(sl.d_buf.data(), b.jobs.d.data(), s, nblk, zs, stages.raw()));
    if ((rc = span_end(c, ev, zs))) return rc;
    HIP_TRY(c, hipMemcpyAsync(b.res.h.data(), b.res.d.data(), (size_t)nblk * sizeof(BzEncRes), hipMemcpyDeviceToHost, zs));
    HIP_TRY(c, hipStreamSynchronize(zs));
    // where every block goes: behind the bits the last slot left
    uint64_t at = z.carry_bits;
    for (uint32_t k = 0; k < nblk; ++k) {
        const BzEncRes& r = b.res.h[k];
        if (r.over || r.bits == 0 || r.bits > (uint64_t)s.slot_words * 32 || r.rle_n == 0 || r.orig_ptr >= r.rle_n)
            return fail(c, SNAPHASH_EDEVICE, "bzip2: a block's stages reported an impossible result");
        b.dst.h[k] = at;
        at += r.bits;
        z.crc = bz_crc_combine(z.crc, crcs[k]);
    }
    const uint64_t out_words = (at + 31) / 32, whole = at / 8;
    if (out_words > b.d_out.size() || out_words * 4 > b.h_out[zbuf].size()) return fail(c, SNAPHASH_EDEVICE, "bzip2: a slot's output outgrew its buffer");
    gz_wait_buf(g, zbuf); // the consumers have let go of what this buffer held two slots ago
    uint8_t* h = b.h_out[zbuf].data();
    HIP_TRY(c, hipMemcpyAsync(b.dst.d.data(), b.dst.h.data(), (size_t)nblk * 8, hipMemcpyHostToDevice, zs));
    if ((rc = span_begin(c, Ev::Codec, zs, &ev2))) return rc;
    HIP_TRY(c, launch_bzenc_concat(s, b.dst.d.data(), nblk, b.d_out.data(), out_words, z.carry, zs));
    if ((rc = span_end(c, ev2, zs))) return rc;
    HIP_TRY(c, hipMemcpyAsync(h, b.d_out.data(), (size_t)out_words * 4, hipMemcpyDeviceToHost, zs));
    HIP_TRY(c, hipStreamSynchronize(zs));
    if (z.self_check && (rc = bz_self_check_slot(g, z, sl, n, nblk, at, out_words, offs, lens, crcs, trace)) != SNAPHASH_OK) return rc;
    if (trace) {
        const float ms[4] = {stages.ms(0), stages.ms(1), stages.ms(2), stages.ms(3)}, cat = span_ms(ev2);
        fprintf(stderr, "snaphash bz2: slot of %llu bytes, %u blocks: crc %.3f ms, rle1 %.3f ms, bwt %.3f ms, mtf %.3f ms, code %.3f ms, concat %.3f ms\n",
                (unsigned long long)n, nblk, crc_ms, ms[0], ms[1], ms[2], ms[3], cat);
    }
    z.carry_bits = (uint32_t)(at & 7);
    z.carry = z.carry_bits ? h[whole] : 0u;
    gz_emit(g, h, whole, zbuf);
    g.st.chunks += nblk;
    return SNAPHASH_OK;
}

int BzEncoder::slot(OutPipe& g, Slot& sl, uint64_t n, hipEvent_t ready, int zbuf, bool is_first, bool is_last)
{
    return bz_process_slot(g, *this, sl, n, ready, zbuf, is_first, is_last);
}

// What the _ex entries were asked for.  opt == nullptr, or an all-zero struct: what the plain entries write (level 9, no
// self-check); otherwise the struct says its size and every field means what it says (level 0 is 9).
int bz2_read_options(snaphash_ctx* x, const snaphash_bz2_options* opt, uint32_t* level, bool* self_check)
{
    *level = 9;
    *self_check = false;
    if (!opt) return SNAPHASH_OK;
    if (opt->struct_size == 0) {
        if (opt->flags || opt->level) return fail(x, SNAPHASH_EINVAL, "snaphash_bz2_options.struct_size");
        return SNAPHASH_OK;
    }
    if (opt->struct_size != sizeof(snaphash_bz2_options)) return fail(x, SNAPHASH_EINVAL, "snaphash_bz2_options.struct_size");
    if (opt->flags & ~(uint32_t)SNAPHASH_BZ2_SELF_CHECK) return fail(x, SNAPHASH_EINVAL, "bzip2: unknown flag");
    *level = bzenc_level(opt->level);
    if (!*level) return fail(x, SNAPHASH_EINVAL, "bzip2: the level is 1 to 9, or 0 for 9");
    *self_check = (opt->flags & SNAPHASH_BZ2_SELF_CHECK) != 0;
    return SNAPHASH_OK;
}

// what snaphash_get_bz2_selfcheck_stats hands out: of this _ex call
void bz2_keep_selfcheck_stats(snaphash_ctx* x, const BzSelfCheck& sc)
{
    x->bz2_selfcheck = snaphash_bz2_selfcheck_stats{};
    x->bz2_selfcheck.struct_size = sizeof(snaphash_bz2_selfcheck_stats);
    x->bz2_selfcheck.blocks = sc.blocks;
    x->bz2_selfcheck.ms = sc.ms;
}

} // namespace

extern "C" {

int snaphash_bzip2_buffer_ex(snaphash_ctx* x, const void* data, size_t n, const snaphash_bz2_options* opt, void** bz_out, size_t* bz_len)
try {
    if (!x || (!data && n) || !bz_out || !bz_len) return fail(x, SNAPHASH_EINVAL, "bad argument");
    *bz_out = nullptr;
    *bz_len = 0;
    uint32_t level;
    bool self;
    int rc = bz2_read_options(x, opt, &level, &self);
    if (rc) return rc;
    BzSelfCheck sc;
    sc.member = "the buffer";
    BzEncoder enc(level, self ? &sc : nullptr);
    rc = encode_to_malloc(x, enc, data, n, bz_out, bz_len);
    bz2_keep_selfcheck_stats(x, sc);
    return rc;
} catch (...) { // allocation or thread-creation failure: no C++ exception crosses the C boundary
    return SNAPHASH_ENOMEM;
}

int snaphash_tar_create_bz2_ex(snaphash_ctx* x, const char* tarname, const char* source_dir, const char* exclude_prefix,
                               const snaphash_bz2_options* opt, char** yaml_out, size_t* yaml_len, uint8_t* archive_digest)
try {
    if (!x || !tarname || !source_dir) return fail(x, SNAPHASH_EINVAL, "bad argument");
    uint32_t level;
    bool self;
    int rc = bz2_read_options(x, opt, &level, &self);
    if (rc) return rc;
    BzSelfCheck sc;
    const char* base = strrchr(tarname, '/');
    sc.member = base ? base + 1 : tarname;
    BzEncoder enc(level, self ? &sc : nullptr);
    rc = tar_create_impl(x, enc, tarname, source_dir, exclude_prefix, nullptr, nullptr, yaml_out, yaml_len, archive_digest);
    bz2_keep_selfcheck_stats(x, sc);
    return rc;
} catch (...) { // allocation or thread-creation failure: no C++ exception crosses the C boundary
    return SNAPHASH_ENOMEM;
}

int snaphash_get_bz2_selfcheck_stats(const snaphash_ctx* x, snaphash_bz2_selfcheck_stats* out)
{
    if (!x || !out || out->struct_size < sizeof(snaphash_bz2_selfcheck_stats)) return SNAPHASH_EINVAL;
    *out = x->bz2_selfcheck;
    out->struct_size = sizeof(snaphash_bz2_selfcheck_stats);
    return SNAPHASH_OK;
}

int snaphash_bz2_check_device(snaphash_ctx* x, const void* d_z, size_t n_z, const uint64_t* z_beg, const uint64_t* z_end, const void* d_in,
                              size_t n_in, const uint64_t* in_off, const uint64_t* in_len, const uint32_t* crc, uint32_t level, size_t n_blocks,
                              snaphash_bz2_verdict* verdicts)
try {
    static_assert(sizeof(snaphash_bz2_verdict) == sizeof(Bz2Verdict), "the verdicts travel as they are");
    if (!x || (n_blocks && (!z_beg || !z_end || !in_off || !in_len || !crc || !verdicts)) || (n_z && !d_z) || (n_in && !d_in))
        return fail(x, SNAPHASH_EINVAL, "bad argument");
    if (level < 1 || level > 9) return fail(x, SNAPHASH_EINVAL, "bzip2: the stream's level is 1 to 9");
    if (n_blocks > 0x7fffffffu) return fail(x, SNAPHASH_EINVAL, "bzip2: too many blocks");
    if (n_blocks == 0) return SNAPHASH_OK;
    TOP_ENTER(x);
    DevCtx* c = x->d0();
    HIP_TRY(c, hipSetDevice(c->device));
    std::vector<Bz2CheckJob> jobs(n_blocks);
    for (size_t k = 0; k < n_blocks; ++k) jobs[k] = Bz2CheckJob{z_beg[k], z_end[k], in_off[k], in_len[k], crc[k], 0};
    DevBuf<Bz2CheckJob> d_jobs;
    DevBuf<Bz2Verdict> d_v;
    HIP_TRY(c, d_jobs.reserve(n_blocks));
    HIP_TRY(c, d_v.reserve(n_blocks));
    HIP_TRY(c, hipMemcpyAsync(d_jobs.data(), jobs.data(), n_blocks * sizeof(Bz2CheckJob), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(d_v.data(), 0xff, n_blocks * sizeof(Bz2Verdict), c->stream));
    const int rc = bz2_check_run(c, (const uint8_t*)d_z, n_z, (const uint8_t*)d_in, n_in, d_jobs.data(), (uint32_t)n_blocks, level, d_v.data(), c->stream,
                                 nullptr);
    const hipError_t e = hipStreamSynchronize(c->stream); // (jobs is read by a copy that may still be in flight)
    if (rc) return lift(x, c, rc);
    HIP_TRY(c, e);
    HIP_TRY(c, hipMemcpy(verdicts, d_v.data(), n_blocks * sizeof(Bz2Verdict), hipMemcpyDeviceToHost));
    x->stats.launches = 5 * ((n_blocks + kBz2CheckGroup - 1) / kBz2CheckGroup);
    end_top(x, t_top0_);
    return SNAPHASH_OK;
} catch (...) { // allocation failure: no C++ exception crosses the C boundary
    return SNAPHASH_ENOMEM;
}

int snaphash_bzip2_buffer(snaphash_ctx* x, const void* data, size_t n, uint32_t level, void** bz_out, size_t* bz_len)
try {
    if (!x || (!data && n) || !bz_out || !bz_len) return fail(x, SNAPHASH_EINVAL, "bad argument");
    *bz_out = nullptr;
    *bz_len = 0;
    level = bzenc_level(level);
    if (!level) return fail(x, SNAPHASH_EINVAL, "bzip2: the level is 1 to 9, or 0 for 9");
    BzEncoder enc(level);
    return encode_to_malloc(x, enc, data, n, bz_out, bz_len);
} catch (...) { // allocation or thread-creation failure: no C++ exception crosses the C boundary
    return SNAPHASH_ENOMEM;
}

int snaphash_bwt_device(snaphash_ctx* x, const void* d_in, const uint64_t* offsets, const uint64_t* lens, size_t n_blocks, void* d_last,
                        void* d_orig_ptr)
try {
    if (!x || (n_blocks && (!d_in || !offsets || !lens || !d_last || !d_orig_ptr))) return fail(x, SNAPHASH_EINVAL, "bad argument");
    uint32_t cap = 0;
    for (size_t i = 0; i < n_blocks; ++i) {
        if (lens[i] < 1 || lens[i] > kBzMaxBlock) return fail(x, SNAPHASH_EINVAL, "bwt: a range is 1 to 900 000 bytes");
        if (lens[i] > ~0ull - offsets[i]) return fail(x, SNAPHASH_EINVAL, "a range wraps around the address space");
        cap = std::max(cap, (uint32_t)lens[i]);
    }
    if (n_blocks == 0) return SNAPHASH_OK;
    TOP_ENTER(x);
    DevCtx* c = x->d0();
    HIP_TRY(c, hipSetDevice(c->device));
    cap = (cap + 63) & ~63u;
    const uint32_t per = (uint32_t)std::min<uint64_t>({(uint64_t)n_blocks, (uint64_t)kBzEncLaunchBlocksMax, std::max<uint64_t>(1, kBzEncLaunchBytes / cap)});
    int rc = ensure_bzenc(c, per, cap, false);
    if (rc) return lift(x, c, rc);
    BzEncBufs& b = c->be;
    const BzEncScratch s = b.scratch();
    for (size_t k0 = 0; k0 < n_blocks; k0 += per) {
        const uint32_t nb = (uint32_t)std::min<size_t>(per, n_blocks - k0);
        for (uint32_t k = 0; k < nb; ++k) b.bwt_jobs.h[k] = BzBwtJob{offsets[k0 + k], offsets[k0 + k], (uint32_t)lens[k0 + k], 0};
        HIP_TRY(c, hipMemcpyAsync(b.bwt_jobs.d.data(), b.bwt_jobs.h.data(), (size_t)nb * sizeof(BzBwtJob), hipMemcpyHostToDevice, c->z_stream));
        HIP_TRY(c, launch_bzenc_bwt((const uint8_t*)d_in, b.bwt_jobs.d.data(), (uint8_t*)d_last, (uint32_t*)d_orig_ptr + k0, s, nb, c->z_stream));
        HIP_TRY(c, hipStreamSynchronize(c->z_stream)); // (the job table is written again for the next launch)
    }
    end_top(x, t_top0_);
    return SNAPHASH_OK;
} catch (...) { // allocation failure: no C++ exception crosses the C boundary
    return SNAPHASH_ENOMEM;
}

// bz_process_slot's sequence once more on a caller's arrays (a copy, as xz_encode_stages is one of xz_process_slot: the
// producer's loop stays as it was): the job table, the CRCs, the four stages -- or, from_last, the last two -- the host's
// placement with its check of the results, the concat kernel.  Only the sort's keys, indices and ranks are the ctx's.
int snaphash_bzenc_stages_device(snaphash_ctx* x, const void* d_in, const uint64_t* offsets, const uint64_t* lens, size_t n_blocks, uint32_t level,
                                 uint32_t cap, uint32_t carry, uint32_t carry_bits, const uint32_t* rle_n, const uint32_t* orig_ptr,
                                 const uint32_t* crc, void* d_rle, void* d_last, void* d_syms, void* d_maps, void* d_sel, void* d_slots, void* d_res,
                                 void* d_dst, void* d_out, size_t out_words, uint64_t* total_bits)
try {
    const bool from_last = rle_n != nullptr;
    if (!x || !total_bits) return fail(x, SNAPHASH_EINVAL, "bad argument");
    *total_bits = 0;
    if (level < 1 || level > 9) return fail(x, SNAPHASH_EINVAL, "bzip2: the level is 1 to 9");
    if (cap == 0) cap = (bzenc_rle_cap(level) + 63) & ~63u;
    if (cap % 64 || cap > ((bzenc_rle_cap(9) + 63) & ~63u)) return fail(x, SNAPHASH_EINVAL, "bzip2: cap is a multiple of 64, at most 899 840, or 0");
    if (carry_bits > 7 || (carry & ~((0xff00u >> carry_bits) & 0xffu)) != 0) // (only the carry_bits highest bits of a byte)
        return fail(x, SNAPHASH_EINVAL, "bzip2: carry is carry_bits < 8 bits, left-aligned in a byte");
    if (n_blocks == 0) {
        *total_bits = carry_bits;
        return SNAPHASH_OK;
    }
    if (!d_last || !d_syms || !d_maps || !d_sel || !d_slots || !d_res || !d_dst || !d_out) return fail(x, SNAPHASH_EINVAL, "bad argument");
    if (from_last ? (!orig_ptr || !crc) : (!d_in || !offsets || !lens || !d_rle)) return fail(x, SNAPHASH_EINVAL, "bad argument");
    if (n_blocks > kBzEncLaunchBlocksMax || n_blocks * (uint64_t)cap > kBzEncLaunchBytes)
        return fail(x, SNAPHASH_EINVAL, "bzip2: more blocks than one launch takes");
    for (size_t k = 0; k < n_blocks; ++k) {
        if (from_last) {
            if (rle_n[k] < 1 || rle_n[k] > cap) return fail(x, SNAPHASH_EINVAL, "bzip2: a last column is 1 to cap bytes");
            if (orig_ptr[k] >= rle_n[k]) return fail(x, SNAPHASH_EINVAL, "bzip2: origPtr is below the column's length");
        } else {
            if (lens[k] < 1 || lens[k] > bzenc_piece(level)) return fail(x, SNAPHASH_EINVAL, "bzip2: a range is 1 byte to the level's piece");
            if (lens[k] > ~0ull - offsets[k]) return fail(x, SNAPHASH_EINVAL, "a range wraps around the address space");
        }
    }
    TOP_ENTER(x);
    DevCtx* c = x->d0();
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t nblk = (uint32_t)n_blocks;
    int rc = ensure_bzenc(c, nblk, cap, false);
    if (rc) return lift(x, c, rc);
    BzEncBufs& b = c->be;
    hipStream_t zs = c->z_stream;
    BzEncScratch s = b.scratch(); // (the sort's scratch: made for at least nblk blocks of cap, walked with this call's stride)
    s.cap = cap;
    s.slot_words = bzenc_slot_words(cap);
    s.rle = (uint8_t*)d_rle; s.last = (uint8_t*)d_last; s.syms = (uint16_t*)d_syms; s.maps = (BzEncMap*)d_maps; s.sel = (uint8_t*)d_sel;
    s.slots = (uint32_t*)d_slots; s.res = (BzEncRes*)d_res;
    std::vector<BzEncRes> res(nblk, BzEncRes{});
    std::vector<uint64_t> dst(nblk);
    std::vector<uint32_t> crcs(nblk);
    if (from_last) {
        for (uint32_t k = 0; k < nblk; ++k) {
            crcs[k] = crc[k];
            res[k].rle_n = rle_n[k];
            res[k].orig_ptr = orig_ptr[k];
            b.jobs.h[k] = BzEncJob{0, 0, crcs[k]};
        }
        HIP_TRY(c, hipMemcpyAsync(b.jobs.d.data(), b.jobs.h.data(), (size_t)nblk * sizeof(BzEncJob), hipMemcpyHostToDevice, zs));
        HIP_TRY(c, hipMemcpyAsync(d_res, res.data(), (size_t)nblk * sizeof(BzEncRes), hipMemcpyHostToDevice, zs));
        HIP_TRY(c, launch_bzenc_from_last(b.jobs.d.data(), s, nblk, zs));
    } else {
        rc = crc_ranges_dev(c, kCrcBzip2, (const uint8_t*)d_in, offsets, lens, nblk, crcs.data(), zs, nullptr);
        if (rc) return lift(x, c, rc);
        for (uint32_t k = 0; k < nblk; ++k) b.jobs.h[k] = BzEncJob{offsets[k], (uint32_t)lens[k], crcs[k]};
        HIP_TRY(c, hipMemcpyAsync(b.jobs.d.data(), b.jobs.h.data(), (size_t)nblk * sizeof(BzEncJob), hipMemcpyHostToDevice, zs));
        HIP_TRY(c, launch_bzenc_blocks((const uint8_t*)d_in, b.jobs.d.data(), s, nblk, zs, nullptr));
    }
    HIP_TRY(c, hipMemcpyAsync(res.data(), d_res, (size_t)nblk * sizeof(BzEncRes), hipMemcpyDeviceToHost, zs));
    HIP_TRY(c, hipStreamSynchronize(zs));
    uint64_t at = carry_bits;
    for (uint32_t k = 0; k < nblk; ++k) {
        const BzEncRes& r = res[k];
        if (r.over || r.bits == 0 || r.bits > (uint64_t)s.slot_words * 32 || r.rle_n == 0 || r.orig_ptr >= r.rle_n)
            return lift(x, c, fail(c, SNAPHASH_EDEVICE, "bzip2: a block's stages reported an impossible result"));
        dst[k] = at;
        at += r.bits;
    }
    if ((at + 31) / 32 > out_words) return lift(x, c, fail(c, SNAPHASH_EINVAL, "bzip2: out_words is smaller than the placed bits need"));
    HIP_TRY(c, hipMemcpyAsync(d_dst, dst.data(), (size_t)nblk * 8, hipMemcpyHostToDevice, zs));
    HIP_TRY(c, launch_bzenc_concat(s, (const uint64_t*)d_dst, nblk, (uint32_t*)d_out, out_words, carry, zs));
    HIP_TRY(c, hipStreamSynchronize(zs));
    *total_bits = at;
    x->stats.launches = (from_last ? 2 : 4) + 1;
    end_top(x, t_top0_);
    return SNAPHASH_OK;
} catch (...) { // allocation failure: no C++ exception crosses the C boundary
    return SNAPHASH_ENOMEM;
}

int snaphash_tar_create_bz2(snaphash_ctx* x, const char* tarname, const char* source_dir, const char* exclude_prefix, char** yaml_out,
                            size_t* yaml_len, uint8_t* archive_digest)
try {
    BzEncoder enc;
    return tar_create_impl(x, enc, tarname, source_dir, exclude_prefix, nullptr, nullptr, yaml_out, yaml_len, archive_digest);
} catch (...) { // allocation or thread-creation failure: no C++ exception crosses the C boundary
    return SNAPHASH_ENOMEM;
}

} // extern "C"
