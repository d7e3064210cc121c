// xzpack.inc -- the data.tar.xz producer, textually part of snaphash_api.cpp (behind targz.inc, whose pass, consumers,
// staging and buffer driver it shares: XzEncoder is one of targz.inc's Encoders, made for a call with the call's parameters).
//
// tarCreate's ".xz" branch (reference clickdeb/deb.go:272-273) pipes the tar stream through `xz --compress --stdout`,
// which writes ONE Block: one serial LZMA chain, for the encoder and for every decoder after it.  Here the staged tar
// stream is cut into Blocks of block_size bytes (1 MiB unless the caller says otherwise) and every Block into LZMA2 chunks
// of 65 536 bytes that reset the coder state but keep the Block's dictionary (xz_enc_core.h): lzma_chains_kernel links
// every Block's hash chains, lzma2_chunks_kernel codes every chunk of the slot side by side, lzma2_concat_kernel puts
// headers and bodies in their final places, and the Blocks' Checks -- CRC-64 unless the caller names CRC-32, SHA-256 or
// none -- come from the kernels the install side uses (crc_kernels.hip, sha256_kernels.hip), over the staged bytes in HBM.
// The host writes what is left: Block headers, padding, Checks, the Index and the footer.  A Block never spans two staging
// slots; a slot's last Block may be short.  The file is one the library's own install side (unxz.inc) decodes a Block a
// thread or a Block a workgroup.  With snaphash_xz_options.filter the LZMA2 kernels read a copy of the slot that
// bcj_kernels.hip has filtered in place, a range a Block (DESIGN.md sec. 25); everything else reads the staged bytes.

namespace {

static_assert(kXzEncBlockMax == kXzGpuBlockMax, "every Block this side writes is one the install side's kernel takes");

// The .xz producer's self-check (DESIGN.md sec. 23), asked for by the _ex entries' SNAPHASH_XZ_SELF_CHECK alone: every slot's
// LZMA2 chunks are walked against the staged stream by lzma2_check_kernel before they leave HBM (lzma2_check_core.h).
struct XzSelfCheck {
    const char* member = ""; // for last_error
    uint64_t chunks = 0;     // chunks checked (all accepted, or the call failed)
    double ms = 0;           // the check kernel's own time, HIP events
    uint64_t bytes = 0;      // of the tar stream, in the slots checked so far
};

// The .xz encoder of one call: the Block size and the Blocks' Check it was asked for (the entries have validated them), and
// the Index records of the Blocks written so far.
struct XzEncoder final : Encoder {
    const uint64_t block_size;
    const uint32_t check;
    std::vector<XzEncRecord> recs;
    XzSelfCheck* const self_check; // null = off, the producer's path without it
    const XzEncChain filter;       // the filters in front of LZMA2 (DESIGN.md sec. 25, 29), none = the producer's path without them
    uint64_t filt_blocks = 0;      // Blocks the BCJ kernels filtered
    double filt_ms = 0;            // the BCJ kernels' own time, HIP events
    const uint32_t level;          // 0: the greedy parse; 1: candidates, prices and a shortest-path parse (DESIGN.md sec. 27)
    explicit XzEncoder(uint64_t bs = kXzEncBlockDefault, uint32_t chk = kXzCheckCrc64, XzSelfCheck* sc = nullptr, XzEncChain flt = XzEncChain(), uint32_t lvl = 0)
        : Encoder(".xz", "xz: the block size is larger than the engine's staging size"), block_size(bs), check(chk), self_check(sc), filter(flt), level(lvl)
    {
        if (sc) check_ms = &sc->ms;
    }
    uint64_t slot_bytes(const DevCtx* c, uint64_t job_bytes) const override // the producer's slot size, cut down to whole Blocks
    {
        const uint64_t s = producer_slot_bytes(c, job_bytes);
        return std::max<uint64_t>(s - s % block_size, block_size);
    }
    int ensure(DevCtx* c, uint64_t slot_bytes) override
    {
        const int rc = ensure_producer_streams(c);
        if (rc) return rc;
        HIP_TRY(c, c->xe.ensure(slot_bytes, c->numa_node)); // (a failure leaves none of it)
        if (level) HIP_TRY(c, c->xe.ensure_level(slot_bytes));
        if (self_check) HIP_TRY(c, c->xe.ensure_check(slot_bytes));
        if (filter) HIP_TRY(c, c->xe.ensure_filter(slot_bytes));
        if (filter && self_check) HIP_TRY(c, c->xe.ensure_filter_check(slot_bytes));
        return SNAPHASH_OK;
    }
    void begin(OutPipe& g) override
    {
        uint8_t h[kXzEncStreamHeader];
        xzenc_stream_header(h, check);
        gz_emit(g, h, sizeof h, -1);
    }
    int slot(OutPipe& g, Slot& sl, uint64_t n, hipEvent_t ready, int zbuf, bool is_first, bool is_last) override;
    int finish(OutPipe& g, uint8_t archive_digest[64]) override // the Index and the footer
    {
        std::vector<uint8_t> tail;
        xzenc_index_footer(recs, tail, check);
        return pipe_finish(g, tail.data(), tail.size(), archive_digest);
    }
};

// The encoder's chain over the first n bytes of d, a range a Block of bs bytes (positions from the Block's first byte), in
// place, queued on zs between ev's two events: a stage of the filter kernels a filter -- encode: the header's first filter
// first; undo: the one nearest LZMA2 first.
int xz_chain_stages(DevCtx* c, const XzEncChain& ch, uint8_t* d, uint64_t n, uint64_t bs, bool encode, hipStream_t zs, const Span& ev)
{
    const uint32_t nblk = (uint32_t)((n + bs - 1) / bs);
    std::vector<BcjRange> fr(nblk);
    HIP_TRY(c, hipEventRecord(ev.a, zs));
    for (uint32_t j = 0; j < ch.n; ++j) {
        const uint32_t f = encode ? j : ch.n - 1 - j;
        for (uint32_t k = 0; k < nblk; ++k)
            fr[k] = BcjRange{(uint64_t)k * bs, std::min<uint64_t>(bs, n - (uint64_t)k * bs), 0, ch.id[f], ch.id[f] == kXzDelta ? ch.param[f] : 0u, encode ? 1u : 0u};
        if (int rc = xz_filter_stage_dev(c, d, fr, encode, zs, nullptr, nullptr)) return rc;
    }
    HIP_TRY(c, hipEventRecord(ev.b, zs));
    return SNAPHASH_OK;
}

// The self-check of a slot, behind lzma2_concat_kernel on the compressor's stream: the chunks' stretches of b.d_out[0 .. total)
// against the slot's staged bytes.  A stretch begins where the host placed the chunk (b.dst) and ends where the host's
// Block layouts say -- the next chunk's place, or the end of the Block's LZMA2 data -- not where the chunk's own header says.
// at[k]: where Block k begins in b.d_out.  Waits for the verdicts; a refused chunk fails the call.  src: the bytes the chunks
// were made from -- the slot's staged bytes, or with a BCJ filter their filtered copy, whose filter is then undone in place
// and the result compared with the staged bytes by the range-compare kernel, a pair a Block.
int xz_self_check_slot(OutPipe& g, XzEncoder& z, Slot& sl, const uint8_t* src, uint64_t n, const std::vector<XzEncBlockLayout>& lay,
                       const std::vector<uint64_t>& at, uint64_t total)
{
    DevCtx* c = g.c;
    XzEncBufs& b = c->xe;
    hipStream_t zs = c->z_stream;
    XzSelfCheck& sc = *z.self_check;
    const uint64_t bs = z.block_size;
    const uint32_t nch = (uint32_t)((n + kXzEncChunk - 1) / kXzEncChunk), cpb = (uint32_t)(bs / kXzEncChunk);
    if (b.zend.size() < nch || b.chk.size() < nch) return fail(c, SNAPHASH_EDEVICE, "xz: the self-check's tables are smaller than the slot");
    for (uint32_t k = 0; k < lay.size(); ++k) {
        const uint64_t blen = std::min<uint64_t>(bs, n - (uint64_t)k * bs);
        const uint32_t ch0 = k * cpb, cn = (uint32_t)((blen + kXzEncChunk - 1) / kXzEncChunk);
        for (uint32_t i = 0; i < cn; ++i) b.zend.h[ch0 + i] = lzma2_check_stretch_end(b.dst.h.data() + ch0, i, cn, at[k] + lay[k].hdr + lay[k].data);
    }
    HIP_TRY(c, hipMemcpyAsync(b.zend.d.data(), b.zend.h.data(), (size_t)nch * 8, hipMemcpyHostToDevice, zs));
    HIP_TRY(c, hipMemsetAsync(b.chk.d.data(), 0xff, (size_t)nch * sizeof(Lzma2Verdict), zs)); // (a verdict that is not written is a refusal)
    for (uint32_t c0 = 0; c0 < nch; c0 += kLzCheckLaunchChunks) {
        Span ev;
        if (int rc = span_begin(c, Ev::Check, zs, &ev)) return rc;
        HIP_TRY(c, launch_lzma2_check(src, n, bs, b.d_out.data(), total, b.dst.d.data(), b.zend.d.data(), c0,
                                      std::min(kLzCheckLaunchChunks, nch - c0), nch, b.chk.d.data(), zs));
        if (int rc = span_end(c, ev, zs)) return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(b.chk.h.data(), b.chk.d.data(), (size_t)nch * sizeof(Lzma2Verdict), hipMemcpyDeviceToHost, zs));
    HIP_TRY(c, hipStreamSynchronize(zs));
    for (uint32_t i = 0; i < nch; ++i) {
        const Lzma2Verdict v = b.chk.h[i];
        if (v.status == kLzCheckOk) continue;
        // (the Block and the chunk count through the whole stream: xz_process_slot calls this BEFORE it adds the slot's
        // Blocks to z.recs and its chunks to g.st.chunks, and sc.bytes grows below; moved behind either, the text would
        // name the wrong Block or chunk)
        return fail(c, SNAPHASH_EDEVICE, lzma2_check_error_text(sc.member, z.recs.size() + i / cpb, g.st.chunks + i, v.status,
                                                               sc.bytes + (uint64_t)i * kXzEncChunk + v.offset));
    }
    if (z.filter) {
        const uint32_t nblk = (uint32_t)lay.size();
        size_t nc = 0;
        for (uint32_t k = 0; k < nblk; ++k) {
            const uint64_t b0 = (uint64_t)k * bs, blen = std::min<uint64_t>(bs, n - b0);
            for (uint64_t off = 0; off < blen; off += kCmpChunk) {
                if (nc >= b.fcmp.size()) return fail(c, SNAPHASH_EDEVICE, "xz: the self-check's tables are smaller than the slot");
                b.fcmp.h[nc++] = CmpChunk{(uint64_t)(uintptr_t)(b.d_filt.data() + b0 + off), (uint64_t)(uintptr_t)(sl.d_buf.data() + b0 + off),
                                          (uint32_t)std::min<uint64_t>(kCmpChunk, blen - off), k};
            }
        }
        if (b.feq.size() < nblk) return fail(c, SNAPHASH_EDEVICE, "xz: the self-check's tables are smaller than the slot");
        Span fev;
        int rc = span_take(c, Ev::Check, &fev);
        if (!rc) rc = xz_chain_stages(c, z.filter, b.d_filt.data(), n, bs, false, zs, fev); // the whole chain undone
        if (rc) return rc;
        HIP_TRY(c, hipMemsetAsync(b.feq.d.data(), 1, nblk, zs)); // equal until a chunk says otherwise
        HIP_TRY(c, hipMemcpyAsync(b.fcmp.d.data(), b.fcmp.h.data(), nc * sizeof(CmpChunk), hipMemcpyHostToDevice, zs));
        HIP_TRY(c, launch_compare(b.fcmp.d.data(), (uint32_t)nc, b.feq.d.data(), zs));
        HIP_TRY(c, hipMemcpyAsync(b.feq.h.data(), b.feq.d.data(), nblk, hipMemcpyDeviceToHost, zs));
        HIP_TRY(c, hipStreamSynchronize(zs));
        z.filt_ms += span_ms(fev);
        for (uint32_t k = 0; k < nblk; ++k) {
            if (b.feq.h[k]) continue;
            // where: the Block's two sides read back (the failing path alone pays for it)
            const uint64_t b0 = (uint64_t)k * bs, blen = std::min<uint64_t>(bs, n - b0);
            std::vector<uint8_t> u(blen), v(blen);
            HIP_TRY(c, hipMemcpy(u.data(), b.d_filt.data() + b0, blen, hipMemcpyDeviceToHost));
            HIP_TRY(c, hipMemcpy(v.data(), sl.d_buf.data() + b0, blen, hipMemcpyDeviceToHost));
            uint64_t off = 0;
            while (off < blen && u[off] == v[off]) ++off;
            char t[256];
            snprintf(t, sizeof t, "xz self-check: %s: Block %llu: the filter undone differs from the staged bytes at offset %llu of the stream", sc.member,
                     (unsigned long long)(z.recs.size() + k), (unsigned long long)(sc.bytes + b0 + off));
            return fail(c, SNAPHASH_EDEVICE, t);
        }
    }
    sc.chunks += nch;
    sc.bytes += n;
    return SNAPHASH_OK;
}

// The slot's first n bytes (in sl.d_buf once `ready` has fired; nullptr: already ordered on the compressor's stream)
// as whole Blocks into c->xe.h_out[zbuf] and on to the consumers.
int xz_process_slot(OutPipe& g, XzEncoder& z, Slot& sl, uint64_t n, hipEvent_t ready, int zbuf, bool, bool)
{
    if (n == 0) return SNAPHASH_OK;
    DevCtx* c = g.c;
    XzEncBufs& b = c->xe;
    hipStream_t zs = c->z_stream;
    const uint64_t bs = z.block_size;
    const uint32_t nch = (uint32_t)((n + kXzEncChunk - 1) / kXzEncChunk), cpb = (uint32_t)(bs / kXzEncChunk);
    const uint32_t nblk = (uint32_t)((n + bs - 1) / bs);
    if (n > sl.cap() || b.d_prev.size() < n || b.res.size() < nch || b.cap() < XzEncBufs::out_cap(n))
        return fail(c, SNAPHASH_EDEVICE, "xz: the encoder's buffers are smaller than the slot");
    if (z.level && b.d_cand_set.size() < n * kXzEncCands) return fail(c, SNAPHASH_EDEVICE, "xz: the encoder's buffers are smaller than the slot");
    uint32_t* const d_cand = z.level ? b.d_cand_set.data() : b.d_cand.data();
    if (ready) HIP_TRY(c, hipStreamWaitEvent(zs, ready, 0));
    // with a BCJ filter: the slot's bytes once more, filtered in place, a range a Block (positions from the Block's first byte);
    // the LZMA2 kernels read the copy, the Checks below the staged bytes
    const uint8_t* src = sl.d_buf.data();
    Span fev, ev, ev2;
    if (z.filter) {
        if (b.d_filt.size() < n) return fail(c, SNAPHASH_EDEVICE, "xz: the encoder's buffers are smaller than the slot");
        HIP_TRY(c, hipMemcpyAsync(b.d_filt.data(), sl.d_buf.data(), n, hipMemcpyDeviceToDevice, zs));
        int frc = span_take(c, Ev::Codec, &fev);
        if (!frc) frc = xz_chain_stages(c, z.filter, b.d_filt.data(), n, bs, true, zs, fev);
        if (frc) return frc;
        src = b.d_filt.data();
        z.filt_blocks += nblk;
    }
    int rc = span_begin(c, Ev::Codec, zs, &ev);
    if (rc) return rc;
    HIP_TRY(c, launch_lzma_chains(src, n, (uint32_t)bs, b.d_prev.data(), zs));
    if ((rc = span_end(c, ev, zs))) return rc;
    // a launch codes what is resident at once, no more: a longer slot goes in several launches (each with its own pair of
    // events: the longest single launch is what DESIGN.md sec. 18 holds against sec. 17's one-second bound)
    std::vector<Span> evl;
    const uint32_t width = z.level ? kXzEncLaunchChunksPriced : kXzEncLaunchChunks;
    for (uint32_t c0 = 0; c0 < nch; c0 += width) {
        evl.emplace_back();
        if ((rc = span_begin(c, Ev::Codec, zs, &evl.back()))) return rc;
        HIP_TRY(c, launch_lzma2_chunks(src, n, (uint32_t)bs, b.d_prev.data(), d_cand, b.d_slots.data(), b.res.d.data(), c0,
                                       std::min(width, nch - c0), zs, z.level));
        if ((rc = span_end(c, evl.back(), zs))) return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(b.res.h.data(), b.res.d.data(), (size_t)nch * 4, hipMemcpyDeviceToHost, zs));
    HIP_TRY(c, hipStreamSynchronize(zs));
    // where everything goes: a Block after the other, a chunk after the other
    std::vector<XzEncBlockLayout> lay(nblk);
    const uint32_t check = z.check, check_size = xzenc_check_size(check);
    std::vector<uint64_t> at(nblk), offs(nblk), lens(nblk);
    std::vector<uint8_t> fields((size_t)nblk * kXzEncCheckMax); // a Block's Check field as the file holds it
    uint64_t total = 0;
    for (uint32_t k = 0; k < nblk; ++k) {
        const uint64_t b0 = (uint64_t)k * bs, blen = std::min<uint64_t>(bs, n - b0);
        const uint32_t ch0 = k * cpb, cn = (uint32_t)((blen + kXzEncChunk - 1) / kXzEncChunk);
        for (uint32_t i = 0; i < cn; ++i) {
            const uint32_t usize = (uint32_t)std::min<uint64_t>(kXzEncChunk, blen - (uint64_t)i * kXzEncChunk);
            if (!xzenc_res_valid(usize, b.res.h[ch0 + i])) return fail(c, SNAPHASH_EDEVICE, "xz: the chunk kernel reported an impossible size");
            g.st.stored_chunks += b.res.h[ch0 + i] == kXzEncStored;
        }
        lay[k] = xzenc_block_layout(b.res.h.data() + ch0, cn, blen, b.dst.h.data() + ch0, check, z.filter);
        for (uint32_t i = 0; i < cn; ++i) b.dst.h[ch0 + i] += total;
        at[k] = total;
        offs[k] = b0;
        lens[k] = blen;
        total += lay[k].total;
    }
    if (total > b.cap()) return fail(c, SNAPHASH_EDEVICE, "xz: a slot's output outgrew its buffer");
    gz_wait_buf(g, zbuf); // the consumers have let go of what this buffer held two slots ago
    uint8_t* h = b.h_out[zbuf].data();
    HIP_TRY(c, hipMemcpyAsync(b.dst.d.data(), b.dst.h.data(), (size_t)nch * 8, hipMemcpyHostToDevice, zs));
    if ((rc = span_begin(c, Ev::Codec, zs, &ev2))) return rc;
    HIP_TRY(c, launch_lzma2_concat(src, n, (uint32_t)bs, b.d_slots.data(), b.res.d.data(), b.dst.d.data(), b.d_out.data(), nch, zs));
    if ((rc = span_end(c, ev2, zs))) return rc;
    HIP_TRY(c, hipMemcpyAsync(h, b.d_out.data(), total, hipMemcpyDeviceToHost, zs));
    // the Blocks' Checks, from the staged bytes in HBM by the Check's kernel (each waits for the stream: the piece is back
    // when it returns; with no Check the stream is waited for here)
    double crc_ms = 0;
    if (check == kXzCheckCrc64) {
        std::vector<uint64_t> crcs(nblk);
        rc = crc_ranges_dev(c, 0, sl.d_buf.data(), offs.data(), lens.data(), nblk, crcs.data(), zs, &crc_ms);
        for (uint32_t k = 0; k < nblk && !rc; ++k) xzenc_le64(fields.data() + (size_t)k * kXzEncCheckMax, crcs[k]);
    } else if (check == kXzCheckCrc32) {
        std::vector<uint32_t> crcs(nblk);
        rc = crc_ranges_dev(c, kCrcGzip, sl.d_buf.data(), offs.data(), lens.data(), nblk, crcs.data(), zs, &crc_ms);
        for (uint32_t k = 0; k < nblk && !rc; ++k) xzenc_le32(fields.data() + (size_t)k * kXzEncCheckMax, crcs[k]);
    } else if (check == kXzCheckSha256) {
        std::vector<uint8_t> dig((size_t)nblk * kSha256Digest);
        rc = sha256_ranges_dev(c, sl.d_buf.data(), offs.data(), lens.data(), nblk, dig.data(), zs, &crc_ms);
        for (uint32_t k = 0; k < nblk && !rc; ++k) memcpy(fields.data() + (size_t)k * kXzEncCheckMax, dig.data() + (size_t)k * kSha256Digest, kSha256Digest);
    } else {
        HIP_TRY(c, hipStreamSynchronize(zs));
    }
    if (rc) return rc;
    float filt_ms = 0;
    if (z.filter) {
        filt_ms = span_ms(fev); // (the stream has been waited for)
        z.filt_ms += filt_ms;
    }
    if (z.self_check && (rc = xz_self_check_slot(g, z, sl, src, n, lay, at, total)) != SNAPHASH_OK) return rc;
    if (getenv("SNAPHASH_TRACE_XZ")) { // the kernels of this slot, one by one (tools/xz_bench.py reads the line)
        const float chains = span_ms(ev), concat = span_ms(ev2);
        float sum = 0, longest = 0;
        for (const Span& e : evl) {
            const float ms = span_ms(e);
            sum += ms;
            longest = std::max(longest, ms);
        }
        fprintf(stderr, "snaphash xz: slot of %llu bytes, %u blocks, %u chunks: chains %.3f ms, chunks %.3f ms in %zu launch(es) (longest %.3f), "
                        "concat %.3f ms, %s %.3f ms\n", (unsigned long long)n, nblk, nch, chains, sum, evl.size(), longest, concat,
                check == kXzCheckSha256 ? "sha256" : check == kXzCheckCrc32 ? "crc32" : check == kXzCheckNone ? "no check" : "crc64", crc_ms);
        if (z.filter) fprintf(stderr, "snaphash xz: slot of %llu bytes: filter 0x%02X %.3f ms\n", (unsigned long long)n, z.filter.first(), filt_ms);
    }
    const uint32_t dict_byte = xzenc_dict_byte(bs);
    for (uint32_t k = 0; k < nblk; ++k) {
        xzenc_block_frame(h + at[k], lay[k], lens[k], dict_byte, fields.data() + (size_t)k * kXzEncCheckMax, check_size, z.filter);
        z.recs.push_back(XzEncRecord{lay[k].unpadded, lens[k]});
    }
    gz_emit(g, h, total, zbuf);
    g.st.chunks += nch;
    return SNAPHASH_OK;
}

int XzEncoder::slot(OutPipe& g, Slot& sl, uint64_t n, hipEvent_t ready, int zbuf, bool is_first, bool is_last)
{
    return xz_process_slot(g, *this, sl, n, ready, zbuf, is_first, is_last);
}

// The producer's kernel sequence once more, for snaphash_xzenc_stages_device: xz_process_slot's steps in its order on a
// caller's buffers (at level 1 d_cand holds kXzEncCands words a byte), without its events and its trace line.  (A copy, not a shared routine: with the sequence shared, the
// producer's call measured above the spread of its parent's on one of three corpora -- DESIGN.md sec. 18 -- so its loop
// stays as it was.)  h_res / h_dst: a word a chunk of host memory.  launch_chunks: 0 for the producer's width at the level.  The concat
// kernel is queued on zs, not waited for.
struct XzEncStageBufs {
    uint32_t *d_prev, *d_cand;
    uint8_t* d_slots;
    uint32_t *d_res, *h_res;
    uint64_t *d_dst, *h_dst;
    uint8_t* d_out;
    uint64_t out_cap;
};
int xz_encode_stages(DevCtx* c, const uint8_t* d_in, uint64_t n, uint64_t bs, uint32_t launch_chunks, const XzEncStageBufs& b, hipStream_t zs,
                     std::vector<XzEncBlockLayout>& lay, uint32_t level)
{
    if (launch_chunks == 0) launch_chunks = level ? kXzEncLaunchChunksPriced : kXzEncLaunchChunks;
    const uint32_t nch = (uint32_t)((n + kXzEncChunk - 1) / kXzEncChunk), cpb = (uint32_t)(bs / kXzEncChunk);
    const uint32_t nblk = (uint32_t)((n + bs - 1) / bs);
    HIP_TRY(c, launch_lzma_chains(d_in, n, (uint32_t)bs, b.d_prev, zs));
    for (uint32_t c0 = 0; c0 < nch; c0 += launch_chunks)
        HIP_TRY(c, launch_lzma2_chunks(d_in, n, (uint32_t)bs, b.d_prev, b.d_cand, b.d_slots, b.d_res, c0, std::min(launch_chunks, nch - c0), zs, level));
    HIP_TRY(c, hipMemcpyAsync(b.h_res, b.d_res, (size_t)nch * 4, hipMemcpyDeviceToHost, zs));
    HIP_TRY(c, hipStreamSynchronize(zs));
    lay.resize(nblk);
    uint64_t total = 0;
    for (uint32_t k = 0; k < nblk; ++k) {
        const uint64_t b0 = (uint64_t)k * bs, blen = std::min<uint64_t>(bs, n - b0);
        const uint32_t ch0 = k * cpb, cn = (uint32_t)((blen + kXzEncChunk - 1) / kXzEncChunk);
        for (uint32_t i = 0; i < cn; ++i) {
            const uint32_t usize = (uint32_t)std::min<uint64_t>(kXzEncChunk, blen - (uint64_t)i * kXzEncChunk);
            if (!xzenc_res_valid(usize, b.h_res[ch0 + i])) return fail(c, SNAPHASH_EDEVICE, "xz: the chunk kernel reported an impossible size");
        }
        lay[k] = xzenc_block_layout(b.h_res + ch0, cn, blen, b.h_dst + ch0);
        for (uint32_t i = 0; i < cn; ++i) b.h_dst[ch0 + i] += total;
        total += lay[k].total;
    }
    if (total > b.out_cap) return fail(c, SNAPHASH_EDEVICE, "xz: a slot's output outgrew its buffer");
    HIP_TRY(c, hipMemcpyAsync(b.d_dst, b.h_dst, (size_t)nch * 8, hipMemcpyHostToDevice, zs));
    HIP_TRY(c, launch_lzma2_concat(d_in, n, (uint32_t)bs, b.d_slots, b.d_res, b.d_dst, b.d_out, nch, zs));
    return SNAPHASH_OK;
}

// the body of snaphash_xz_buffer / snaphash_xz_buffer_check
int xz_buffer_entry(snaphash_ctx* x, const void* data, size_t n, uint64_t block_size, uint32_t check, void** xz_out, size_t* xz_len)
try {
    if (!x || (!data && n) || !xz_out || !xz_len) return fail(x, SNAPHASH_EINVAL, "bad argument");
    *xz_out = nullptr;
    *xz_len = 0;
    if (!xzenc_check_valid(check)) return fail(x, SNAPHASH_EINVAL, "xz: the Check is 0 (none), 1 (CRC-32), 4 (CRC-64) or 10 (SHA-256)");
    if (!xzenc_block_size(&block_size)) return fail(x, SNAPHASH_EINVAL, "xz: the block size is a multiple of 64 KiB from 64 KiB to 4 MiB, or 0");
    XzEncoder enc(block_size, check);
    return encode_to_malloc(x, enc, data, n, xz_out, xz_len);
} catch (...) { // allocation or thread-creation failure: no C++ exception crosses the C boundary
    return SNAPHASH_ENOMEM;
}

constexpr uint32_t kXzOptionsSizeV1 = 24; // snaphash_xz_options before level and reserved2
constexpr uint32_t kXzOptionsSizeV2 = 32; // before chain_len and chain
constexpr uint32_t kXzOptionsSizeV3 = 48;

// What the _ex entries were asked for.  opt == nullptr, or an all-zero struct: what the plain entries write (1 MiB, CRC-64, no
// self-check); otherwise the struct says its size and every field means what it says (check 0 is "none").
int xz_read_options(snaphash_ctx* x, const snaphash_xz_options* opt, uint64_t* block_size, uint32_t* check, bool* self_check, XzEncChain* filter,
                    uint32_t* level)
{
    static_assert(sizeof(snaphash_xz_options) == kXzOptionsSizeV3 && offsetof(snaphash_xz_options, level) == kXzOptionsSizeV1 &&
                      offsetof(snaphash_xz_options, chain_len) == kXzOptionsSizeV2,
                  "level and reserved2 behind the 24 bytes, the chain behind the 32");
    *block_size = kXzEncBlockDefault;
    *check = kXzCheckCrc64;
    *self_check = false;
    *filter = XzEncChain();
    *level = 0;
    if (opt && opt->struct_size == 0) { // (the plain entry: only the 24 bytes every caller has are looked at)
        if (opt->flags || opt->block_size || opt->check || opt->filter) return fail(x, SNAPHASH_EINVAL, "snaphash_xz_options.struct_size");
        return SNAPHASH_OK;
    }
    if (!opt) return SNAPHASH_OK;
    // 24: the struct before it had a level (level 0); 32 and more: with level and reserved2; 48 and more: with a chain
    if (opt->struct_size != kXzOptionsSizeV1 && opt->struct_size < kXzOptionsSizeV2) return fail(x, SNAPHASH_EINVAL, "snaphash_xz_options.struct_size");
    if (opt->struct_size >= kXzOptionsSizeV2) {
        if (opt->level > kXzEncLevelMax) return fail(x, SNAPHASH_EINVAL, "xz: the level is 0 (greedy parse) or 1 (priced parse)");
        if (opt->reserved2) return fail(x, SNAPHASH_EINVAL, "xz: snaphash_xz_options.reserved2 is not 0");
        *level = opt->level;
    }
    if (opt->flags & ~(uint32_t)SNAPHASH_XZ_SELF_CHECK) return fail(x, SNAPHASH_EINVAL, "xz: unknown flag");
    if (!xzenc_filter_valid(opt->filter)) return fail(x, SNAPHASH_EINVAL, "xz: the filter is 0 (none), 4 (x86), 7 (ARM) or 8 (ARM-Thumb)");
    if (!xzenc_check_valid(opt->check)) return fail(x, SNAPHASH_EINVAL, "xz: the Check is 0 (none), 1 (CRC-32), 4 (CRC-64) or 10 (SHA-256)");
    *block_size = opt->block_size;
    if (!xzenc_block_size(block_size)) return fail(x, SNAPHASH_EINVAL, "xz: the block size is a multiple of 64 KiB from 64 KiB to 4 MiB, or 0");
    *check = opt->check;
    *self_check = (opt->flags & SNAPHASH_XZ_SELF_CHECK) != 0;
    *filter = XzEncChain(opt->filter);
    if (opt->struct_size >= kXzOptionsSizeV3 && opt->chain_len) {
        XzEncChain ch;
        ch.n = opt->chain_len;
        for (uint32_t k = 0; k < 3 && k < ch.n; ++k) {
            ch.id[k] = opt->chain[k] & 0xff;
            ch.param[k] = opt->chain[k] >> 8;
        }
        if (opt->filter) return fail(x, SNAPHASH_EINVAL, "xz: filter and chain_len are both set");
        if (!xzenc_chain_valid(ch))
            return fail(x, SNAPHASH_EINVAL, "xz: the chain is up to 3 filters, each an id 3 .. 9, Delta (3) with a distance of 1 .. 256 in the bits above the id, the others with 0");
        *filter = ch;
    }
    return SNAPHASH_OK;
}

// what snaphash_get_xz_selfcheck_stats hands out: of this _ex call
void xz_keep_selfcheck_stats(snaphash_ctx* x, const XzSelfCheck& sc)
{
    x->xz_selfcheck = snaphash_xz_selfcheck_stats{};
    x->xz_selfcheck.struct_size = sizeof(snaphash_xz_selfcheck_stats);
    x->xz_selfcheck.chunks = sc.chunks;
    x->xz_selfcheck.ms = sc.ms;
}

// what snaphash_get_xz_filter_stats hands out: of this _ex call
void xz_keep_filter_stats(snaphash_ctx* x, const XzEncoder& z)
{
    x->xz_filter = snaphash_xz_filter_stats{};
    x->xz_filter.struct_size = sizeof(snaphash_xz_filter_stats);
    x->xz_filter.filter = z.filter.first(); // (the id the header names first)
    x->xz_filter.device_blocks = z.filt_blocks;
    x->xz_filter.device_ms = z.filt_ms;
}

} // namespace

extern "C" {

int snaphash_xz_buffer_ex(snaphash_ctx* x, const void* data, size_t n, const snaphash_xz_options* opt, void** xz_out, size_t* xz_len)
try {
    if (!x || (!data && n) || !xz_out || !xz_len) return fail(x, SNAPHASH_EINVAL, "bad argument");
    *xz_out = nullptr;
    *xz_len = 0;
    uint64_t bs;
    uint32_t check;
    bool self;
    XzEncChain filter;
    uint32_t level;
    int rc = xz_read_options(x, opt, &bs, &check, &self, &filter, &level);
    if (rc) return rc;
    XzSelfCheck sc;
    sc.member = "the buffer";
    XzEncoder enc(bs, check, self ? &sc : nullptr, filter, level);
    rc = encode_to_malloc(x, enc, data, n, xz_out, xz_len);
    xz_keep_selfcheck_stats(x, sc);
    xz_keep_filter_stats(x, enc);
    return rc;
} catch (...) { // allocation or thread-creation failure: no C++ exception crosses the C boundary
    return SNAPHASH_ENOMEM;
}

int snaphash_tar_create_xz_ex(snaphash_ctx* x, const char* tarname, const char* source_dir, const char* exclude_prefix,
                              const snaphash_xz_options* opt, char** yaml_out, size_t* yaml_len, uint8_t* archive_digest)
try {
    if (!x || !tarname || !source_dir) return fail(x, SNAPHASH_EINVAL, "bad argument");
    uint64_t bs;
    uint32_t check;
    bool self;
    XzEncChain filter;
    uint32_t level;
    int rc = xz_read_options(x, opt, &bs, &check, &self, &filter, &level);
    if (rc) return rc;
    XzSelfCheck sc;
    const char* base = strrchr(tarname, '/');
    sc.member = base ? base + 1 : tarname;
    XzEncoder enc(bs, check, self ? &sc : nullptr, filter, level);
    rc = tar_create_impl(x, enc, tarname, source_dir, exclude_prefix, nullptr, nullptr, yaml_out, yaml_len, archive_digest);
    xz_keep_selfcheck_stats(x, sc);
    xz_keep_filter_stats(x, enc);
    return rc;
} catch (...) { // allocation or thread-creation failure: no C++ exception crosses the C boundary
    return SNAPHASH_ENOMEM;
}

int snaphash_get_xz_selfcheck_stats(const snaphash_ctx* x, snaphash_xz_selfcheck_stats* out)
{
    if (!x || !out || out->struct_size < sizeof(snaphash_xz_selfcheck_stats)) return SNAPHASH_EINVAL;
    *out = x->xz_selfcheck;
    out->struct_size = sizeof(snaphash_xz_selfcheck_stats);
    return SNAPHASH_OK;
}

int snaphash_lzma2_check_device(snaphash_ctx* x, const void* d_in, size_t n_in, uint64_t block_size, const void* d_z, size_t n_z,
                                const uint64_t* z_beg, const uint64_t* z_end, size_t nchunks, uint32_t launch_chunks,
                                snaphash_lzma2_verdict* verdicts)
try {
    static_assert(sizeof(snaphash_lzma2_verdict) == sizeof(Lzma2Verdict), "the verdicts travel as they are");
    static_assert(kLzCheckLaunchChunks == kXzEncLaunchChunks && kLzCheckChunk == kXzEncChunk && kLzCheckProbs == kXzEncProbs &&
                      kLzCheckProps == kXzEncProps,
                  "the check walks what the producer writes");
    if (!x || !d_in || !z_beg || !z_end || !verdicts || n_in == 0 || (n_z && !d_z)) return fail(x, SNAPHASH_EINVAL, "bad argument");
    if (!xzenc_block_size(&block_size)) return fail(x, SNAPHASH_EINVAL, "xz: the block size is a multiple of 64 KiB from 64 KiB to 4 MiB, or 0");
    if (nchunks != (n_in + kLzCheckChunk - 1) / kLzCheckChunk || nchunks > 0x7fffffffu) return fail(x, SNAPHASH_EINVAL, "xz: nchunks is not ceil(n_in / 65536)");
    if (launch_chunks > kLzCheckLaunchChunks) return fail(x, SNAPHASH_EINVAL, "xz: a launch holds at most 2048 chunks");
    if (launch_chunks == 0) launch_chunks = kLzCheckLaunchChunks;
    TOP_ENTER(x);
    DevCtx* c = x->d0();
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<uint64_t> d_tab; // z_beg, then z_end
    DevBuf<Lzma2Verdict> d_v;
    HIP_TRY(c, d_tab.reserve(2 * nchunks));
    HIP_TRY(c, d_v.reserve(nchunks));
    HIP_TRY(c, hipMemcpyAsync(d_tab.data(), z_beg, nchunks * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_tab.data() + nchunks, z_end, nchunks * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(d_v.data(), 0xff, nchunks * sizeof(Lzma2Verdict), c->stream));
    uint64_t launches = 0;
    for (size_t c0 = 0; c0 < nchunks; c0 += launch_chunks, ++launches)
        HIP_TRY(c, launch_lzma2_check((const uint8_t*)d_in, n_in, block_size, (const uint8_t*)d_z, n_z, d_tab.data(), d_tab.data() + nchunks, (uint32_t)c0,
                                      (uint32_t)std::min<size_t>(launch_chunks, nchunks - c0), (uint32_t)nchunks, d_v.data(), c->stream));
    HIP_TRY(c, hipMemcpyAsync(verdicts, d_v.data(), nchunks * sizeof(Lzma2Verdict), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    x->stats.launches = launches;
    end_top(x, t_top0_);
    return SNAPHASH_OK;
} catch (...) { // allocation failure: no C++ exception crosses the C boundary
    return SNAPHASH_ENOMEM;
}

int snaphash_xz_buffer(snaphash_ctx* x, const void* data, size_t n, uint64_t block_size, void** xz_out, size_t* xz_len)
{
    return xz_buffer_entry(x, data, n, block_size, kXzCheckCrc64, xz_out, xz_len);
}

int snaphash_xz_buffer_check(snaphash_ctx* x, const void* data, size_t n, uint64_t block_size, uint32_t check, void** xz_out, size_t* xz_len)
{
    return xz_buffer_entry(x, data, n, block_size, check, xz_out, xz_len);
}

int snaphash_xzenc_stages_device(snaphash_ctx* x, const void* d_in, size_t n, uint64_t block_size, uint32_t launch_chunks, void* d_prev,
                                 void* d_cand, void* d_slots, void* d_res, void* d_dst, void* d_out, size_t out_cap, uint64_t* block_total)
{
    return snaphash_xzenc_stages_device_ex(x, d_in, n, block_size, launch_chunks, d_prev, d_cand, d_slots, d_res, d_dst, d_out, out_cap, block_total, 0);
}

int snaphash_xzenc_stages_device_ex(snaphash_ctx* x, const void* d_in, size_t n, uint64_t block_size, uint32_t launch_chunks, void* d_prev,
                                    void* d_cand, void* d_slots, void* d_res, void* d_dst, void* d_out, size_t out_cap, uint64_t* block_total,
                                    uint32_t level)
try {
    if (level > kXzEncLevelMax) return fail(x, SNAPHASH_EINVAL, "xz: the level is 0 (greedy parse) or 1 (priced parse)");
    if (!x || (n && (!d_in || !d_prev || !d_cand || !d_slots || !d_res || !d_dst || !d_out))) return fail(x, SNAPHASH_EINVAL, "bad argument");
    if (!xzenc_block_size(&block_size)) return fail(x, SNAPHASH_EINVAL, "xz: the block size is a multiple of 64 KiB from 64 KiB to 4 MiB, or 0");
    if (launch_chunks > kXzEncLaunchChunks) return fail(x, SNAPHASH_EINVAL, "xz: a launch holds at most 2048 chunks");
    if (n > ((uint64_t)0x7fffffffu - 1) * kXzEncChunk) return fail(x, SNAPHASH_EINVAL, "xz: the piece is too long");
    if (n == 0) return SNAPHASH_OK;
    if (out_cap < XzEncBufs::out_cap(n)) return fail(x, SNAPHASH_EINVAL, "xz: out_cap is smaller than a piece of n bytes may need");
    TOP_ENTER(x);
    DevCtx* c = x->d0();
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t nch = (size_t)((n + kXzEncChunk - 1) / kXzEncChunk);
    std::vector<uint32_t> h_res(nch);
    std::vector<uint64_t> h_dst(nch);
    const XzEncStageBufs sb = {(uint32_t*)d_prev, (uint32_t*)d_cand, (uint8_t*)d_slots, (uint32_t*)d_res, h_res.data(),
                               (uint64_t*)d_dst, h_dst.data(), (uint8_t*)d_out, out_cap};
    std::vector<XzEncBlockLayout> lay;
    const int rc = xz_encode_stages(c, (const uint8_t*)d_in, n, block_size, launch_chunks, sb, c->stream, lay, level);
    const hipError_t e = hipStreamSynchronize(c->stream); // (h_dst is read by a copy still in flight)
    if (rc) return lift(x, c, rc);
    HIP_TRY(c, e);
    if (block_total)
        for (size_t k = 0; k < lay.size(); ++k) block_total[k] = lay[k].total;
    end_top(x, t_top0_);
    return SNAPHASH_OK;
} catch (...) { // allocation failure: no C++ exception crosses the C boundary
    return SNAPHASH_ENOMEM;
}

int snaphash_tar_create_xz(snaphash_ctx* x, const char* tarname, const char* source_dir, const char* exclude_prefix, char** yaml_out,
                           size_t* yaml_len, uint8_t* archive_digest)
try {
    XzEncoder enc;
    return tar_create_impl(x, enc, tarname, source_dir, exclude_prefix, nullptr, nullptr, yaml_out, yaml_len, archive_digest);
} catch (...) { // allocation or thread-creation failure: no C++ exception crosses the C boundary
    return SNAPHASH_ENOMEM;
}

} // extern "C"
