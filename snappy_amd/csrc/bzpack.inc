// bzpack.inc -- the data.tar.bz2 producer, textually part of snaphash_api.cpp (behind targz.inc, whose pass, consumers,
// staging and buffer driver it shares: BzEncoder is one of targz.inc's Encoders, as xzpack.inc's XzEncoder is).
//
// The reference's tarCreate refuses a ".bz2" name (clickdeb/deb.go:274-275) and snaphash_tar_create keeps doing so; this
// is the writer of the one format the install side reads (ClickDeb.Unpack, deb.go:185) and the library could not write.
// The staged tar stream is cut into pieces of bzenc_piece(level) bytes, a bzip2 block each (bzip2_enc_core.h), and a
// staging slot is a whole number of pieces, no more than one launch codes: the blocks' CRCs come from crc_kernels.hip over
// the staged bytes, bzip2_enc_kernels.hip runs RLE1, the BWT, MTF and the Huffman coding of every block of the slot side by
// side and shifts their bits together.  The host adds the four bytes in front and the footer, folds the combined CRC, and
// holds the stream's last partial byte back until the next slot (or the footer) completes it.

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

// The .bz2 encoder of one call: the level it was asked for (1 to 9), the combined CRC so far, and the stream's last, partial
// byte -- held back until the next slot's blocks (or the footer) complete it.
struct BzEncoder final : Encoder {
    const uint32_t level;
    uint32_t crc = 0, carry = 0, carry_bits = 0;
    explicit BzEncoder(uint32_t lvl = 9) : Encoder(".bz2", "bzip2: a block's input is larger than the engine's staging size"), level(lvl) {}
    uint64_t slot_bytes(const DevCtx* c, uint64_t job_bytes) const override { return bz_slot_bytes(c, job_bytes, level); }
    int ensure(DevCtx* c, uint64_t slot_bytes) override { return ensure_bzenc(c, (uint32_t)(slot_bytes / bzenc_piece(level)), bzenc_rle_cap(level), true); }
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
    hipEvent_t stage_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int i = 0; i < 5; ++i) if (e[i]) (void)hipEventDestroy(e[i]); } } evg{stage_ev};
    if (trace)
        for (hipEvent_t& e : stage_ev) HIP_TRY(c, hipEventCreate(&e));
    EventPair* evp = next_events(c, 2);
    if (!evp) return fail(c, SNAPHASH_EDEVICE, "hipEventCreate failed");
    const EventPair ev = *evp; // (by value: the pool may grow)
    HIP_TRY(c, hipEventRecord(ev.a, zs));
    HIP_TRY(c, launch_bzenc_blocks(sl.d_buf.data(), b.jobs.d.data(), s, nblk, zs, trace ? stage_ev : nullptr));
    HIP_TRY(c, hipEventRecord(ev.b, zs));
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
    EventPair* evp2 = next_events(c, 2);
    if (!evp2) return fail(c, SNAPHASH_EDEVICE, "hipEventCreate failed");
    const EventPair ev2 = *evp2;
    HIP_TRY(c, hipEventRecord(ev2.a, zs));
    HIP_TRY(c, launch_bzenc_concat(s, b.dst.d.data(), nblk, b.d_out.data(), out_words, z.carry, zs));
    HIP_TRY(c, hipEventRecord(ev2.b, zs));
    HIP_TRY(c, hipMemcpyAsync(h, b.d_out.data(), (size_t)out_words * 4, hipMemcpyDeviceToHost, zs));
    HIP_TRY(c, hipStreamSynchronize(zs));
    if (trace) {
        float ms[4] = {0, 0, 0, 0}, cat = 0;
        for (int i = 0; i < 4; ++i) (void)hipEventElapsedTime(&ms[i], stage_ev[i], stage_ev[i + 1]);
        (void)hipEventElapsedTime(&cat, ev2.a, ev2.b);
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

} // namespace

extern "C" {

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

int snaphash_tar_create_bz2(snaphash_ctx* x, const char* tarname, const char* source_dir, const char* exclude_prefix, char** yaml_out,
                            size_t* yaml_len, uint8_t* archive_digest)
try {
    BzEncoder enc;
    return tar_create_impl(x, enc, tarname, source_dir, exclude_prefix, nullptr, nullptr, yaml_out, yaml_len, archive_digest);
} catch (...) { // allocation or thread-creation failure: no C++ exception crosses the C boundary
    return SNAPHASH_ENOMEM;
}

} // extern "C"
