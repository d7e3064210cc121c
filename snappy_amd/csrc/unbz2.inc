// unbz2.inc -- the data.tar.bz2 side of the install path, textually part of snaphash_api.cpp (after unpack.inc, which
// owns DecodedStream and everything behind the decoder; this file owns the bzip2 decoder and its codec entry, kBunzip2Codec).
//
// The reference's ClickDeb.Unpack takes data.tar.{gz,bz2,xz} (clickdeb/deb.go:185); skipToArMember (deb.go:408-441)
// reads the .bz2 member with Go's compress/bzip2, in-process on one core.  Here a bzip2 stream is decoded block by block
// side by side -- on host threads in the default configuration, by the GPU kernels (bzip2_kernels.hip) under
// SNAPHASH_FLAG_GPU_ONLY -- and the decoded stream goes through the same unpack and in-pass Verify as data.tar.gz.

namespace {

// A launch's slots hold the BWT bytes (then the inverse BWT's output), the T vector and the RLE1 chunk states of one
// block each: 4.5 MB.  kBzLaunchSlots of them (1.2 GB) bound the scratch whatever the input; a larger input takes more
// launches.  The piece (compressed bytes a launch's candidates come from) is at most the staging size, 64 MiB.
constexpr uint32_t kBzLaunchSlots = 256;
static_assert(kBz2CheckGroup <= kBzLaunchSlots, "the producer's self-check (bzpack.inc) takes groups no larger than this side's batch");

// the scratch of a job, sized for it; on any allocation failure none is left behind
int ensure_bzip2(DevCtx* c, uint64_t piece, uint32_t slots)
{
    const int rc = DecodedStream::stream(c);
    if (rc) return rc;
    HIP_TRY(c, c->bz.ensure(piece, slots, c->numa_node));
    return SNAPHASH_OK;
}

// The later stages of the nb linked blocks in c->bz.h_blk (their stored CRCs in crcs): the inverse BWT and the RLE1 count,
// the blocks' output offsets by a prefix sum here, the RLE1 write at those offsets in c->inf.d_out (where ds says the
// run begins), the bytes back to ds.out, and every block's CRC checked on host threads, one block each
// (bz_crc_block runs at about 0.4 GB/s a core: the host threads keep pace with the kernels; DESIGN.md sec. 15).
// crc_at = CrcAt::Device: the blocks' CRCs by the CRC kernels instead, a range a block at the offsets the RLE1 stage wrote
// them to, before the bytes travel back.
int bunzip2_batch(snaphash_ctx* x, DevCtx* c, uint32_t nb, const std::vector<uint32_t>& crcs, DecodedStream& ds, snaphash_unpack_stats& st,
                  float& kms, CrcAt crc_at, CrcTally* tally)
{
    std::vector<uint8_t>& out = ds.out;
    HIP_TRY(c, hipMemcpyAsync(c->bz.d_blk.data(), c->bz.h_blk.data(), (size_t)nb * sizeof(BzGpuBlock), hipMemcpyHostToDevice, c->f_stream));
    Span ev;
    int rc = span_begin(c, Ev::Codec, c->f_stream, &ev);
    if (rc) return rc;
    HIP_TRY(c, launch_bz_ibwt(c->bz.d_slots.data(), c->bz.d_tt.data(), c->bz.d_blk.data(), nb, c->f_stream));
    HIP_TRY(c, launch_bz_rle1_count(c->bz.d_slots.data(), c->bz.d_blk.data(), c->bz.d_chunks.data(), nb, c->f_stream));
    if ((rc = span_end(c, ev, c->f_stream))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->bz.h_blk.data(), c->bz.d_blk.data(), (size_t)nb * sizeof(BzGpuBlock), hipMemcpyDeviceToHost, c->f_stream));
    HIP_TRY(c, hipStreamSynchronize(c->f_stream));
    kms += span_ms(ev);
    const size_t o0 = out.size();
    const uint64_t base = ds.dev_base(o0);
    uint64_t total = 0;
    for (uint32_t i = 0; i < nb; ++i) {
        // (a broken inverse BWT walk; a corrupt block that walks leaves it to the block CRC, as libbz2 and Go do)
        if (c->bz.h_blk[i].status != kBzOk) return fail(c, SNAPHASH_EFORMAT, "bzip2: corrupt block (inverse BWT)");
        c->bz.h_blk[i].out_off = base + total;
        total += c->bz.h_blk[i].out_len;
    }
    rc = ds.reserve_dev(c, base + total, base);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->bz.d_blk.data(), c->bz.h_blk.data(), (size_t)nb * sizeof(BzGpuBlock), hipMemcpyHostToDevice, c->f_stream));
    if ((rc = span_begin(c, Ev::Codec, c->f_stream, &ev))) return rc;
    HIP_TRY(c, launch_bz_rle1_write(c->bz.d_slots.data(), c->bz.d_blk.data(), c->bz.d_chunks.data(), nb, c->inf.d_out.data(), c->f_stream));
    if ((rc = span_end(c, ev, c->f_stream))) return rc;
    out.resize(o0 + total);
    rc = ds.fetch(o0, o0, o0 + total);
    if (!rc) rc = ds.sync();
    if (rc) return rc;
    kms += span_ms(ev);
    if (crc_at == CrcAt::Device) {
        std::vector<uint64_t> offs(nb), lens(nb);
        for (uint32_t i = 0; i < nb; ++i) { offs[i] = c->bz.h_blk[i].out_off; lens[i] = c->bz.h_blk[i].out_len; }
        std::vector<uint32_t> got(nb);
        double ms = 0;
        rc = crc_ranges_dev(c, kCrcBzip2, c->inf.d_out.data(), offs.data(), lens.data(), nb, got.data(), c->f_stream, &ms);
        if (rc) return rc;
        if (tally) { tally->device_ranges += nb; tally->device_ms += ms; }
        if (got != crcs) return fail(c, SNAPHASH_EFORMAT, "bzip2: block CRC mismatch");
        st.segments += nb;
        st.gpu_segments += nb;
        scratch_spans_done(c);
        return SNAPHASH_OK;
    }
    if (tally) tally->host_ranges += nb;
    std::atomic<uint32_t> next{0}, bad{0};
    auto work = [&]() {
        for (;;) {
            const uint32_t i = next.fetch_add(1);
            if (i >= nb) return;
            const BzGpuBlock& B = c->bz.h_blk[i];
            if (bz_crc_block(out.data() + o0 + (B.out_off - base), B.out_len) != crcs[i]) bad.store(1);
        }
    };
    {
        const unsigned T = (unsigned)std::min<uint64_t>(nb, call_cpus(x));
        ThreadJoiner th;
        for (unsigned k = 1; k < T; ++k) th.spawn(work);
        work();
        th.join_all();
    }
    if (bad.load()) return fail(c, SNAPHASH_EFORMAT, "bzip2: block CRC mismatch");
    st.segments += nb;
    st.gpu_segments += nb;
    scratch_spans_done(c);
    return SNAPHASH_OK;
}

// Decodes every stream of bz[0..n) and appends the bytes to ds.out; keep_dev: the whole decoded stream also stays in
// c->inf.d_out[0..out.size()) for Verify's device hashing, as gunzip_engine leaves it.
int bunzip2_engine(snaphash_ctx* x, DevCtx* c, const uint8_t* bz, size_t n, DecodedStream& ds, snaphash_unpack_stats& st, CrcAt crc_at,
                   CrcTally* tally)
{
    if (n == 0) return fail(c, SNAPHASH_EFORMAT, "bzip2: empty stream");
    std::vector<uint8_t>& out = ds.out;
    c->fout_gen++;
    const unsigned cpus = call_cpus(x);
    if (!x->gpu_only && cpus >= 2) {
        // the default configuration: the blocks on host threads wherever two cores are there to take them (measured
        // 7.5-11x one core of libbz2 with 16 cores, the kernels 2.6-5.7x: DESIGN.md sec. 15); on one core the kernels,
        // which beat it; SNAPHASH_FLAG_GPU_ONLY sends every linked block through the kernels
        uint64_t blocks = 0;
        if (bzip2_host_threads(bz, n, out, cpus, &blocks)) {
            ds.rollback();
            return fail(c, SNAPHASH_EFORMAT, "bzip2: corrupt stream");
        }
        st.segments += blocks;
        st.host_bytes += out.size() - ds.o_start;
        if (tally) tally->host_ranges += blocks;
        return ds.mirror(ds.o_start, out.size());
    }
    BzCursor cur;
    cur.in = bz;
    cur.n = n;
    if (bz_cursor_stream(cur, 0)) return fail(c, SNAPHASH_EFORMAT, "bzip2: not a bzip2 stream");
    const uint64_t P = std::min<uint64_t>(std::max<uint64_t>(c->staging, 4u << 20), 64ull << 20);
    int rc = ensure_bzip2(c, std::min<uint64_t>(P, n), 8);
    if (rc) return rc;
    std::unique_ptr<BzScratch> hs; // the host decoder's, for a block the kernels do not take
    float kms = 0;
    auto host_block = [&]() -> int { // the block at cur.bit by the host decoder
        if (!hs) hs.reset(new BzScratch);
        const size_t o0 = out.size();
        const BzBlockRes r = bz_block_host(bz, n, cur.bit, cur.level * 100000u, *hs, out);
        if (r.status != kBzOk) return fail(c, SNAPHASH_EFORMAT, "bzip2: corrupt block");
        bz_cursor_take(cur, r.end_bit, r.crc);
        st.segments++;
        st.host_bytes += out.size() - o0;
        if (tally) tally->host_ranges++; // (the host decoder checks its block's CRC itself)
        return ds.mirror(o0, out.size());
    };
    bool chain_order = false; // more candidates than the cap: one block a launch, in chain order
    for (;;) {
        int k = bz_cursor_next(cur);
        if (k < 0) return fail(c, SNAPHASH_EFORMAT, "bzip2: bad stream framing or combined CRC");
        if (k == 0) break;
        // a piece: the compressed bytes from the byte that holds the next block's first bit
        const uint64_t pb = cur.bit >> 3;
        const uint64_t pn = std::min<uint64_t>(chain_order ? std::min<uint64_t>(P, 4u << 20) : P, n - pb);
        HIP_TRY(c, hipMemcpyAsync(c->bz.d_in.data(), bz + pb, pn, hipMemcpyHostToDevice, c->f_stream));
        std::vector<uint64_t> cand;
        if (!chain_order) {
            HIP_TRY(c, hipMemsetAsync(c->bz.d_count.data(), 0, 4, c->f_stream));
            Span ev;
            if ((rc = span_begin(c, Ev::Codec, c->f_stream, &ev))) return rc;
            HIP_TRY(c, launch_bz_scan(c->bz.d_in.data(), pn, c->bz.d_cand.data(), c->bz.d_count.data(), (uint32_t)c->bz.cand_cap(), c->f_stream));
            if ((rc = span_end(c, ev, c->f_stream))) return rc;
            HIP_TRY(c, hipMemcpyAsync(c->bz.h_count.data(), c->bz.d_count.data(), 4, hipMemcpyDeviceToHost, c->f_stream));
            HIP_TRY(c, hipStreamSynchronize(c->f_stream));
            kms += span_ms(ev);
            if (c->bz.h_count[0] > c->bz.cand_cap()) {
                chain_order = true;
            } else if (c->bz.h_count[0]) {
                HIP_TRY(c, hipMemcpyAsync(c->bz.h_cand.data(), c->bz.d_cand.data(), (size_t)c->bz.h_count[0] * 8, hipMemcpyDeviceToHost, c->f_stream));
                HIP_TRY(c, hipStreamSynchronize(c->f_stream));
                cand.assign(c->bz.h_cand.data(), c->bz.h_cand.data() + c->bz.h_count[0]);
                std::sort(cand.begin(), cand.end());
            }
        }
        const uint64_t rel0 = cur.bit - pb * 8;
        if (chain_order) cand.assign(1, rel0);
        size_t idx = (size_t)(std::lower_bound(cand.begin(), cand.end(), rel0) - cand.begin());
        if (idx == cand.size() || cand[idx] != rel0) { // (the chain's block is no candidate: cannot happen below the cap)
            rc = host_block();
            if (rc) return rc;
            continue;
        }
        bool piece_done = false, finished = false;
        while (!piece_done && !finished) {
            // the symbol stage of the next launch's candidates, from the one the chain is at
            const uint32_t K = (uint32_t)std::min<size_t>(cand.size() - idx, kBzLaunchSlots);
            rc = ensure_bzip2(c, std::min<uint64_t>(P, n), std::max<uint32_t>(K, 8));
            if (rc) return rc;
            memcpy(c->bz.h_cand.data(), cand.data() + idx, (size_t)K * 8);
            HIP_TRY(c, hipMemcpyAsync(c->bz.d_cand.data(), c->bz.h_cand.data(), (size_t)K * 8, hipMemcpyHostToDevice, c->f_stream));
            Span ev;
            if ((rc = span_begin(c, Ev::Codec, c->f_stream, &ev))) return rc;
            HIP_TRY(c, launch_bz_symbols(c->bz.d_in.data(), pn, c->bz.d_cand.data(), K, c->bz.d_slots.data(), c->bz.d_res.data(), c->f_stream));
            if ((rc = span_end(c, ev, c->f_stream))) return rc;
            HIP_TRY(c, hipMemcpyAsync(c->bz.h_res.data(), c->bz.d_res.data(), (size_t)K * sizeof(BzBlockRes), hipMemcpyDeviceToHost, c->f_stream));
            HIP_TRY(c, hipStreamSynchronize(c->f_stream));
            kms += span_ms(ev);
            const uint64_t* lc = cand.data() + idx;
            for (;;) { // link what this launch decoded, then run the linked blocks through the later stages
                uint32_t nb = 0;
                std::vector<uint32_t> crcs;
                bool host_next = false;
                for (;;) {
                    k = bz_cursor_next(cur);
                    if (k < 0) return fail(c, SNAPHASH_EFORMAT, "bzip2: bad stream framing or combined CRC");
                    if (k == 0) { finished = true; break; }
                    const uint64_t rel = cur.bit - pb * 8;
                    const uint64_t* it = std::lower_bound(lc, lc + K, rel);
                    if (cur.bit < pb * 8 || it == lc + K || *it != rel) { // past this launch: the next launch or piece
                        const size_t at = (size_t)(std::lower_bound(cand.begin(), cand.end(), rel) - cand.begin());
                        if (cur.bit >= pb * 8 && at < cand.size() && cand[at] == rel) idx = at;
                        else piece_done = true;
                        break;
                    }
                    const uint32_t j = (uint32_t)(it - lc);
                    const BzBlockRes& r = c->bz.h_res[j];
                    if (r.status != kBzOk || r.n > cur.level * 100000u) {
                        // a block the piece cuts off starts the next piece; anything else is the host decoder's
                        if (r.status == kBzTruncated && pb + pn < n && rel > 7) { piece_done = true; break; }
                        host_next = true;
                        break;
                    }
                    BzGpuBlock& B = c->bz.h_blk[nb++];
                    B.out_off = 0; B.out_len = 0; B.slot = j; B.n = r.n; B.orig_ptr = r.orig_ptr; B.status = kBzOk;
                    crcs.push_back(r.crc);
                    bz_cursor_take(cur, r.end_bit + pb * 8, r.crc);
                }
                if (nb) {
                    rc = bunzip2_batch(x, c, nb, crcs, ds, st, kms, crc_at, tally);
                    if (rc) return rc;
                }
                if (!host_next) break;
                rc = host_block();
                if (rc) return rc;
            }
            if (!finished && !piece_done && idx >= cand.size()) piece_done = true;
        }
        if (finished) break;
    }
    scratch_spans_done(c);
    st.inflate_ms += kms;
    return SNAPHASH_OK;
}

const UnpackCodec kBunzip2Codec = {"bzip2", bunzip2_engine};

} // namespace

extern "C" {

int snaphash_bunzip2_buffer(snaphash_ctx* x, const void* bz, size_t n, void** out, size_t* out_len)
{
    return decode_to_malloc(x, kBunzip2Codec, bz, n, out, out_len);
}

int snaphash_tar_unpack_bz2(snaphash_ctx* x, const char* data_tar_bz2, const char* target_dir, const char* yaml, size_t yaml_len,
                            snaphash_mismatch* first, uint8_t* archive_digest)
{
    return tar_unpack_entry(x, kBunzip2Codec, data_tar_bz2, target_dir, yaml, yaml_len, first, archive_digest);
}

} // extern "C"
