// unpack.inc -- the install side (SURVEY sec. 8 row f5), textually part of snaphash_api.cpp (it uses the engine's
// streams, events, the hashing kernels and Verify's comparison).  It owns what every data-member format shares --
// DecodedStream (where decoded bytes live, on the host and in HBM), the codec table's type, the member writer (the tar
// reader it trusts is tar_core.h, host-only), the members' digests and the Verify tail -- and the gzip decoder; unbz2.inc and unxz.inc add a decoder each,
// snap.inc the .snap session that drives them.
//
// The reference unpacks a package with ClickDeb.Unpack (clickdeb/deb.go:188-203): gzip.NewReader (deb.go:427) -- one Go
// inflate on one core -- into helpers.UnpackTar (helpers/helpers.go:74-147) with clickVerifyContentFn (deb.go:96-103);
// the Verify hook (snappy/click.go:955-970) then reads every file of the unpacked tree again.  Here the archive is
// decoded by the GPU inflate (inflate_kernels.hip) into HBM, written out from there, and -- with hashes.yaml -- every
// regular member is hashed out of the decoded stream that is already in HBM: nothing is read back from disk.

#include "tar_core.h"

namespace {

// Where a decoder's bytes live.  Every decoder appends to `out`; with keep_dev the same bytes also sit in c->inf.d_out
// at the same offset (Verify's SHA-512 kernels and the CRC kernels read them there).  Without keep_dev d_out is scratch:
// a run of bytes the kernels decode starts at its offset 0 and nothing a host thread decoded goes there.  Every copy and
// kernel of the install side runs on c->f_stream.
struct DecodedStream {
    DevCtx* c;
    std::vector<uint8_t>& out;
    const bool keep_dev;
    const size_t o_start; // out.size() when the decode began
    DecodedStream(DevCtx* c_, std::vector<uint8_t>& out_, bool keep_dev_) : c(c_), out(out_), keep_dev(keep_dev_), o_start(out_.size()) {}

    static int stream(DevCtx* c)
    {
        HIP_TRY(c, c->f_stream.ensure(hipStreamNonBlocking));
        return SNAPHASH_OK;
    }
    // d_out of `end` bytes or more; `keep` bytes of what is there are kept when it grows
    static int reserve_dev(DevCtx* c, uint64_t end, uint64_t keep)
    {
        DevBuf<uint8_t>& d = c->inf.d_out;
        if (d.size() >= end) return SNAPHASH_OK;
        uint64_t cap = std::max<uint64_t>(end, d.size() + d.size() / 2);
        cap = (cap + (1u << 20) - 1) & ~(uint64_t)((1u << 20) - 1);
        DevBuf<uint8_t> p;
        HIP_TRY(c, p.reserve(cap));
        if (keep && d.data()) {
            const hipError_t e = hipMemcpyAsync(p.data(), d.data(), keep, hipMemcpyDeviceToDevice, c->f_stream);
            if (e == hipSuccess) (void)hipStreamSynchronize(c->f_stream);
            HIP_TRY(c, e);
        }
        d = std::move(p);
        return SNAPHASH_OK;
    }
    // a whole decoded stream into d_out from offset 0 (a session whose stream another decode has overwritten)
    static int upload(DevCtx* c, const std::vector<uint8_t>& bytes)
    {
        int rc = stream(c);
        if (!rc) rc = reserve_dev(c, std::max<size_t>(bytes.size(), 1), 0);
        if (rc) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->inf.d_out.data(), bytes.data(), bytes.size(), hipMemcpyHostToDevice, c->f_stream));
        HIP_TRY(c, hipStreamSynchronize(c->f_stream));
        return SNAPHASH_OK;
    }

    // the offset in d_out of out[run0], where a run of bytes the kernels decode begins
    uint64_t dev_base(size_t run0) const { return keep_dev ? run0 : 0; }
    // host-decoded out[from..to) into HBM at the same offset: nothing without keep_dev
    int mirror_async(size_t from, size_t to)
    {
        if (!keep_dev || to <= from) return SNAPHASH_OK;
        int rc = stream(c);
        if (!rc) rc = reserve_dev(c, to, from);
        if (rc) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->inf.d_out.data() + from, out.data() + from, to - from, hipMemcpyHostToDevice, c->f_stream));
        return SNAPHASH_OK;
    }
    int mirror(size_t from, size_t to)
    {
        const int rc = mirror_async(from, to);
        return rc || !keep_dev || to <= from ? rc : sync();
    }
    // kernel-decoded out[from..to) of the run that began at out[run0], back from HBM; the caller syncs
    int fetch(size_t run0, size_t from, size_t to)
    {
        if (to > from) HIP_TRY(c, hipMemcpyAsync(out.data() + from, c->inf.d_out.data() + dev_base(run0) + (from - run0), to - from, hipMemcpyDeviceToHost, c->f_stream));
        return SNAPHASH_OK;
    }
    int sync()
    {
        HIP_TRY(c, hipStreamSynchronize(c->f_stream));
        return SNAPHASH_OK;
    }
    void rollback() { out.resize(o_start); } // a corrupt stream leaves nothing behind
};

// the compressed piece (and its candidates) and the segments a launch decodes
int ensure_inflate(DevCtx* c, uint64_t piece, uint32_t slots, uint32_t slot_syms = kInflateSlotSyms, uint64_t bcand = 0,
                   uint32_t host_bslots = 0)
{
    const int rc = DecodedStream::stream(c);
    if (rc) return rc;
    HIP_TRY(c, c->inf.ensure(piece, slots, c->numa_node, slot_syms, bcand, host_bslots));
    return SNAPHASH_OK;
}

// Where a decoder takes the CRCs it checks.  Host: on host threads, out of the decoded bytes in host memory (every entry
// point before the .snap session, and the session in the default configuration).  Device: by crc_kernels.hip out of the
// decoded stream in c->inf.d_out -- the session's choice under SNAPHASH_FLAG_GPU_ONLY (snap.inc).
enum class CrcAt { Host, Device };
struct CrcTally { // what a session's decodes did about their CRCs
    uint64_t device_ranges = 0, host_ranges = 0;
    double device_ms = 0; // the CRC kernels, HIP events
};

// A data-member format of the install side (ClickDeb.Unpack's data.tar.{gz,bz2,xz}, deb.go:185): its decoder appends the
// decoded stream to ds.  kGunzipCodec below, kBunzip2Codec in unbz2.inc, kUnxzCodec in unxz.inc.
struct UnpackCodec {
    const char* name;
    int (*decode)(snaphash_ctx*, DevCtx*, const uint8_t*, size_t, DecodedStream&, snaphash_unpack_stats&, CrcAt, CrcTally*);
};

// ---- block mode (SNAPHASH_FLAG_SPLIT_BLOCKS, DESIGN.md sec. 14) ----------------------------------------------------------

// A member that starts with less than this left of the stream takes the serial route.  A member's length is not known
// before it is decoded, so block mode begins each member with a piece of this size, then takes full pieces: a small
// member followed by others costs one such scan, not a scan of the rest of the stream.  (Doubling from here instead cost
// the GPU-only decode a launch per step, each as long as its slowest block: measured slower than the serial route.)  (A choice: at this size
// the block route already beats the serial one, DESIGN.md sec. 14; smaller sizes were not measured.)
constexpr uint64_t kSplitMinBytes = 1u << 20;
constexpr uint64_t kInflateBlockScratch = 1200000000; // the block slots and the piece in HBM (GPU-only), at most
constexpr uint32_t kHostBlockSlots = 256;             // candidates a piece of the host-thread decode takes (InflateBufs h_bslots)
constexpr uint64_t kBlockPiecePerSlot = 16u << 10;    // compressed bytes a slot stands for: zlib's blocks took 12-31 KB

// The linked segments' holes filled on the GPU (one pass over all, then -- if holes are left -- the segments that hold them
// in order) and their symbols laid end to end into the decoded bytes: appended to ds.out and, with keep_dev, left in HBM.
// 1: holes are left (cannot happen after the ordered sweep: the caller falls back to the host decoder).
int gpu_fill_concat(DevCtx* c, uint32_t nl, uint64_t total, uint32_t slot_syms, DecodedStream& ds, size_t m0, bool trace,
                    float& kms)
{
    std::vector<uint8_t>& out = ds.out;
    const size_t o0 = out.size();
    const uint32_t wlen = (uint32_t)std::min<size_t>(kInfWindow, o0 - m0);
    if (wlen) HIP_TRY(c, hipMemcpyAsync(c->inf.d_win.data(), out.data() + o0 - wlen, wlen, hipMemcpyHostToDevice, c->f_stream));
    HIP_TRY(c, hipMemcpyAsync(c->inf.d_links.data(), c->inf.h_links.data(), (size_t)nl * sizeof(InflateLink), hipMemcpyHostToDevice, c->f_stream));
    bool filled = false;
    Span ev;
    for (int pass = 0; pass < 2 && !filled; ++pass) {
        HIP_TRY(c, hipMemsetAsync(c->inf.d_flags.data(), 0, 8, c->f_stream));
        if (int rc = span_begin(c, Ev::Codec, c->f_stream, &ev)) return rc;
        if (pass == 1)
            for (uint32_t j = 0; j < nl; ++j)
                if (c->inf.h_links[j].hole_end) HIP_TRY(c, launch_inflate_fill(c->inf.d_slots.data(), slot_syms, c->inf.d_links.data(), j, 1, c->inf.d_win.data(), wlen, c->inf.d_flags.data(), c->f_stream));
        if (pass == 1) HIP_TRY(c, hipMemsetAsync(c->inf.d_flags.data(), 0, 8, c->f_stream));
        HIP_TRY(c, launch_inflate_fill(c->inf.d_slots.data(), slot_syms, c->inf.d_links.data(), 0, nl, c->inf.d_win.data(), wlen, c->inf.d_flags.data(), c->f_stream));
        if (int rc = span_end(c, ev, c->f_stream)) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->inf.h_flags.data(), c->inf.d_flags.data(), 8, hipMemcpyDeviceToHost, c->f_stream));
        HIP_TRY(c, hipStreamSynchronize(c->f_stream));
        kms += span_ms(ev);
        if (c->inf.h_flags[1]) return fail(c, SNAPHASH_EFORMAT, "gzip: a back-reference before the start of the member");
        filled = c->inf.h_flags[0] == 0;
        if (trace) fprintf(stderr, "snaphash inflate: fill pass %d: %u holes left\n", pass, c->inf.h_flags[0]);
    }
    if (!filled) return 1;
    int rc = ds.reserve_dev(c, ds.dev_base(o0) + total, ds.dev_base(o0));
    if (rc) return rc;
    if ((rc = span_begin(c, Ev::Codec, c->f_stream, &ev))) return rc;
    HIP_TRY(c, launch_inflate_concat(c->inf.d_slots.data(), slot_syms, c->inf.d_links.data(), nl, c->inf.d_out.data() + ds.dev_base(o0), c->f_stream));
    if ((rc = span_end(c, ev, c->f_stream))) return rc;
    out.resize(o0 + total);
    rc = ds.fetch(o0, o0, o0 + total);
    if (!rc) rc = ds.sync();
    if (rc) return rc;
    kms += span_ms(ev);
    return 0;
}

// One member's raw DEFLATE stream z[0..zn) in block mode, appended to ds.out (the member's output starts at m0).  Pieces
// start at any bit: the block scan and the stored-block scan on the GPU give the candidates, every candidate is decoded
// into a slot (the inflate kernel under SNAPHASH_FLAG_GPU_ONLY, host threads otherwise), the chain is linked from the
// piece's start bit and filled in order.  Where it breaks at the piece's start the host decoder takes the stretch to the
// next block the scan can find.  *final_bit: where the final block ended.
int gunzip_blocks(snaphash_ctx* x, DevCtx* c, const uint8_t* z, uint64_t zn, DecodedStream& ds, size_t m0, snaphash_unpack_stats& st,
                  float& kms, uint64_t* final_bit)
{
    std::vector<uint8_t>& out = ds.out;
    snaphash_block_scan_stats& bs = x->block_scan;
    const bool host_mode = !x->gpu_only;
    static const bool trace = getenv("SNAPHASH_TRACE_INFLATE") != nullptr;
    const uint64_t P0 = std::min<uint64_t>(std::max<uint64_t>(c->staging, 64u << 10), kInflateBlockPieceMax);
    // the slots within the scratch cap (the piece and its candidates come first), and the piece from the slots
    const uint64_t per_slot = 2ull * kInflateBlockSlotSyms + 2 * sizeof(InflateSegRes) + 2 * sizeof(InflateLink);
    // (and no more than the stream needs: blocks take 15 KB of input or more, a slot per 4 KiB leaves room for false starts)
    const uint32_t S = host_mode ? kHostBlockSlots
                                 : (uint32_t)std::min<uint64_t>({4096, (kInflateBlockScratch - 2 * P0) / per_slot, std::min(zn, P0) / 4096 + 64});
    const uint64_t P = std::min<uint64_t>(P0, (uint64_t)S * kBlockPiecePerSlot);
    const uint64_t bcap = P / 64 + 4096;
    int rc = ensure_inflate(c, std::min<uint64_t>(P, zn), host_mode ? 64 : S, host_mode ? kInflateSlotSyms : kInflateBlockSlotSyms, bcap,
                            host_mode ? kHostBlockSlots : 0);
    if (rc) return rc;
    const uint32_t slots = host_mode ? kHostBlockSlots : c->inf.nslots(kInflateBlockSlotSyms);
    uint16_t* hsl = c->inf.h_bslots.data(); // host mode: the slots (symbols) and the bytes narrowed from them
    uint8_t* hby = c->inf.h_bbytes.data();
    std::vector<InflateSegRes> hres(host_mode ? kHostBlockSlots : 0);
    uint64_t cur = 0;                                // bit in z where the next segment starts
    uint64_t piece = std::min<uint64_t>(P, kSplitMinBytes); // the member's first piece: its end is not known yet
    for (;;) {
        const uint64_t b0 = cur >> 3, sb = cur & 7, pn = std::min<uint64_t>(piece, zn - b0);
        piece = P;
        // the scans: block headers at every bit, stored-block ends at every byte
        HIP_TRY(c, hipMemcpyAsync(c->inf.d_in.data(), z + b0, pn, hipMemcpyHostToDevice, c->f_stream));
        HIP_TRY(c, hipMemsetAsync(c->inf.d_cand.data(), 0, 4, c->f_stream));
        HIP_TRY(c, hipMemsetAsync(c->inf.d_bcand.data(), 0, 4, c->f_stream));
        Span ev, evb; // the block scan's own time, within both scans'
        if ((rc = span_begin(c, Ev::Codec, c->f_stream, &ev))) return rc;
        HIP_TRY(c, launch_inflate_scan(c->inf.d_in.data(), pn, c->inf.d_cand.data() + 1, c->inf.d_cand.data(), (uint32_t)c->inf.cand_cap(), c->f_stream));
        if ((rc = span_begin(c, Ev::Codec, c->f_stream, &evb))) return rc;
        HIP_TRY(c, launch_inflate_block_scan(c->inf.d_in.data(), pn, c->inf.d_bcand.data() + 1, c->inf.d_bcand.data(), (uint32_t)c->inf.bcand_cap(), c->f_stream));
        if ((rc = span_end(c, evb, c->f_stream)) || (rc = span_end(c, ev, c->f_stream))) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->inf.h_cand.data(), c->inf.d_cand.data(), 4, hipMemcpyDeviceToHost, c->f_stream));
        HIP_TRY(c, hipMemcpyAsync(c->inf.h_bcand.data(), c->inf.d_bcand.data(), 4, hipMemcpyDeviceToHost, c->f_stream));
        HIP_TRY(c, hipStreamSynchronize(c->f_stream));
        kms += span_ms(ev);
        bs.scan_ms += span_ms(evb);
        const uint64_t ns = std::min<uint64_t>(c->inf.h_cand[0], c->inf.cand_cap());
        const uint64_t nb = std::min<uint64_t>(c->inf.h_bcand[0], c->inf.bcand_cap());
        if (ns) HIP_TRY(c, hipMemcpyAsync(c->inf.h_cand.data() + 1, c->inf.d_cand.data() + 1, ns * 4, hipMemcpyDeviceToHost, c->f_stream));
        if (nb) HIP_TRY(c, hipMemcpyAsync(c->inf.h_bcand.data() + 1, c->inf.d_bcand.data() + 1, nb * 4, hipMemcpyDeviceToHost, c->f_stream));
        HIP_TRY(c, hipStreamSynchronize(c->f_stream));
        bs.bits_scanned += pn * 8;
        bs.candidates += c->inf.h_bcand[0];
        // the candidates in order from the piece's start bit: block starts, stored-block ends, the start itself
        std::vector<uint32_t> blocks(c->inf.h_bcand.data() + 1, c->inf.h_bcand.data() + 1 + nb);
        std::sort(blocks.begin(), blocks.end());
        std::vector<uint32_t> cand;
        cand.reserve(nb + ns + 1);
        cand.push_back((uint32_t)sb);
        for (uint32_t v : blocks)
            if (v > sb) cand.push_back(v);
        for (uint64_t k = 0; k < ns; ++k)
            if (c->inf.h_cand[1 + k] > 0) cand.push_back(c->inf.h_cand[1 + k] * 8);
        std::sort(cand.begin(), cand.end());
        cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
        if (cand.size() > slots) cand.resize(slots); // (past the launch's slots the piece is cut)
        const uint32_t K = (uint32_t)cand.size();
        auto is_block = [&](uint64_t bit) { return std::binary_search(blocks.begin(), blocks.end(), (uint32_t)bit); };
        uint32_t nl = 0, from_block = 0;
        uint64_t pos = sb;
        bool fin = false;
        if (host_mode) {
            // as the flush mode's host path: workers decode every candidate into its slot, this thread links and fills
            std::unique_ptr<std::atomic<uint32_t>[]> done(new std::atomic<uint32_t>[K]);
            for (uint32_t i = 0; i < K; ++i) done[i].store(0, std::memory_order_relaxed);
            std::atomic<uint32_t> next{0};
            const uint8_t* zp = z + b0;
            auto work = [&]() {
                InflateTables t;
                for (;;) {
                    const uint32_t i = next.fetch_add(1);
                    if (i >= K) return;
                    uint16_t* sy = hsl + (size_t)i * kInflateBlockSlotSyms;
                    const InflateRun r = inflate_run<uint16_t>(zp, pn, cand[i], sy, 0, kInflateBlockSlotSyms, true, false, t, kInflateBlockMinOut);
                    uint8_t* by = hby + (size_t)i * kInflateBlockSlotSyms;
                    uint32_t last = 0;
                    for (uint32_t q = 0; q < (uint32_t)r.out_len; ++q) {
                        by[q] = (uint8_t)sy[q];
                        last = sy[q] >= kInfHole ? q + 1 : last;
                    }
                    hres[i] = InflateSegRes{r.end_bit, (uint32_t)r.out_len, last, r.status, (uint32_t)r.cut};
                    done[i].store(1, std::memory_order_release);
                }
            };
            const unsigned T = (unsigned)std::min<uint64_t>(K, std::max(2u, call_cpus(x)) - 1);
            ThreadJoiner th;
            for (unsigned k = 0; k < T; ++k) th.spawn(work);
            const size_t o0 = out.size();
            bool bad = false;
            for (;;) {
                const auto it = std::lower_bound(cand.begin(), cand.end(), (uint32_t)pos);
                if (it == cand.end() || *it != pos) break;
                const uint32_t i = (uint32_t)(it - cand.begin());
                while (!done[i].load(std::memory_order_acquire)) std::this_thread::yield();
                const InflateSegRes& r = hres[i];
                if (r.status != kInfBlock && r.status != kInfFinal) break;
                const size_t base = out.size();
                out.resize(base + r.out_len);
                memcpy(out.data() + base, hby + (size_t)i * kInflateBlockSlotSyms, r.out_len);
                if (!fill_holes_host(hsl + (size_t)i * kInflateBlockSlotSyms, r.hole_end, out.data() + base, base - m0)) { bad = true; break; }
                ++nl;
                from_block += is_block(pos);
                if (r.status == kInfFinal) { fin = true; *final_bit = r.end_bit + b0 * 8; break; }
                pos = r.end_bit;
                if (pos >= pn * 8) break;
            }
            next.store(K); // (what is left of the piece is scanned and decoded again as the next piece)
            th.join_all();
            if (bad) return fail(c, SNAPHASH_EFORMAT, "gzip: a back-reference before the start of the member");
            rc = ds.mirror(o0, out.size());
            if (rc) return rc;
        } else {
            memcpy(c->inf.h_cand.data() + 1, cand.data(), (size_t)K * 4);
            HIP_TRY(c, hipMemcpyAsync(c->inf.d_cand.data() + 1, c->inf.h_cand.data() + 1, (size_t)K * 4, hipMemcpyHostToDevice, c->f_stream));
            if ((rc = span_begin(c, Ev::Codec, c->f_stream, &ev))) return rc;
            HIP_TRY(c, launch_inflate_decode_blocks(c->inf.d_in.data(), pn, c->inf.d_cand.data() + 1, K, c->inf.d_slots.data(), c->inf.d_res.data(), c->f_stream));
            if ((rc = span_end(c, ev, c->f_stream))) return rc;
            HIP_TRY(c, hipMemcpyAsync(c->inf.h_res.data(), c->inf.d_res.data(), (size_t)K * sizeof(InflateSegRes), hipMemcpyDeviceToHost, c->f_stream));
            HIP_TRY(c, hipStreamSynchronize(c->f_stream));
            kms += span_ms(ev);
            uint64_t off = 0;
            for (;;) {
                const auto it = std::lower_bound(cand.begin(), cand.end(), (uint32_t)pos);
                if (it == cand.end() || *it != pos) break;
                const uint32_t i = (uint32_t)(it - cand.begin());
                const InflateSegRes& r = c->inf.h_res[i];
                if (r.status != kInfBlock && r.status != kInfFinal) break;
                InflateLink& L = c->inf.h_links[nl++];
                L.off = off;
                L.slot = i;
                L.len = r.out_len;
                L.hole_end = r.hole_end;
                L.pad = 0;
                off += r.out_len;
                from_block += is_block(pos);
                if (r.status == kInfFinal) { fin = true; *final_bit = r.end_bit + b0 * 8; break; }
                pos = r.end_bit;
                if (pos >= pn * 8) break;
            }
            if (nl) {
                rc = gpu_fill_concat(c, nl, off, kInflateBlockSlotSyms, ds, m0, trace, kms);
                if (rc < 0) return rc;
                if (rc) { nl = 0; fin = false; } // (holes left: the host decoder takes over from the piece's start)
                else st.gpu_segments += nl;
            }
        }
        if (trace)
            fprintf(stderr, "snaphash inflate blocks: piece at bit %llu, %llu bytes, %llu block + %llu stored candidates, chain of %u, stopped at bit %llu%s\n",
                    (unsigned long long)cur, (unsigned long long)pn, (unsigned long long)nb, (unsigned long long)ns, nl,
                    (unsigned long long)pos, fin ? " (final)" : "");
        bs.linked += from_block;
        bs.unreached += c->inf.h_bcand[0] - from_block;
        st.segments += nl;
        scratch_spans_done(c);
        if (fin) return 0;
        if (nl) {
            cur = b0 * 8 + pos;
            continue;
        }
        // the chain breaks at the piece's start: the host decoder to the next block end a segment can start from
        const size_t o0 = out.size();
        const InflateRun r = inflate_host_append(z, zn, cur, out, m0, false, 0);
        if (r.status != kInfFinal && !(r.status == kInfBlock && r.end_bit > cur)) return fail(c, SNAPHASH_EFORMAT, "gzip: corrupt DEFLATE stream");
        st.segments++;
        st.host_bytes += out.size() - o0;
        bs.host_blocks++;
        rc = ds.mirror(o0, out.size());
        if (rc) return rc;
        if (r.status == kInfFinal) { *final_bit = r.end_bit; return 0; }
        cur = r.end_bit;
    }
}

// Decodes every gzip member of gz[0..n) and appends the bytes to ds.out; keep_dev: the whole decoded stream also stays in
// c->inf.d_out[0..out.size()).  Pieces of at most c->staging compressed bytes; each ends on a segment boundary and the
// member's last 32 KiB of output travel to the next as its window.
// crc_at = CrcAt::Device (honoured with keep_dev, where the whole stream is in HBM): every member's CRC-32 is taken by the CRC
// kernels when the last member is decoded, a range a member, instead of by crc_parallel member by member; tally (may be
// null) counts what was taken where.
int gunzip_engine(snaphash_ctx* x, DevCtx* c, const uint8_t* gz, size_t n, DecodedStream& ds, snaphash_unpack_stats& st, CrcAt crc_at,
                  CrcTally* tally)
{
    if (n == 0) return fail(c, SNAPHASH_EFORMAT, "gzip: empty stream");
    std::vector<uint8_t>& out = ds.out;
    c->fout_gen++;
    const bool dev_crc = crc_at == CrcAt::Device && ds.keep_dev;
    std::vector<uint64_t> m_off, m_len; // dev_crc: the members' ranges of the decoded stream and their stored CRC-32s
    std::vector<uint32_t> m_crc;
    x->block_scan = snaphash_block_scan_stats{};
    x->block_scan.struct_size = sizeof(snaphash_block_scan_stats);
    const bool split = (x->flags & SNAPHASH_FLAG_SPLIT_BLOCKS) != 0;
    const uint64_t P = std::min<uint64_t>(std::max<uint64_t>(c->staging, 64u << 10), 64ull << 20);
    const uint32_t S = (uint32_t)std::min<uint64_t>(4096, std::max<uint64_t>(64, P / 16384));
    int rc = ensure_inflate(c, std::min<uint64_t>(P, n), (uint32_t)std::min<uint64_t>(S, std::max<uint64_t>(64, n / 4096 + 1)));
    if (rc) return rc;
    const uint32_t slots = c->inf.nslots();
    static const bool trace = getenv("SNAPHASH_TRACE_INFLATE") != nullptr; // the pieces and their chains on stderr
    const bool host_mode = !x->gpu_only;
    constexpr uint64_t kHostPiece = 8u << 20; // compressed bytes a piece of the host-thread decode takes (its slots: 2 B a symbol)
    std::vector<uint16_t> hslots;
    std::vector<uint8_t> hbytes;
    float kms = 0;
    if (n >= 18) { // the output in one allocation: ISIZE of the last member (exact for a single member under 4 GiB)
        const uint64_t isize = gz[n - 4] | (uint64_t)gz[n - 3] << 8 | (uint64_t)gz[n - 2] << 16 | (uint64_t)gz[n - 1] << 24;
        if (isize <= (uint64_t)n * 1032) out.reserve(out.size() + (size_t)isize);
    }
    size_t at = 0;
    while (at < n) {
        size_t h = 0;
        if (gzip_header(gz + at, n - at, &h)) return fail(c, SNAPHASH_EFORMAT, "gzip: bad member header");
        const uint8_t* z = gz + at + h;
        const uint64_t zn = n - at - h;
        const size_t m0 = out.size();
        uint64_t cur = 0; // byte offset in z where the next segment starts
        uint64_t final_bit = 0;
        bool ended = false;
        // the host decoder from cur to the next segment end (or the member's end)
        auto host_run = [&]() -> int {
            const size_t o0 = out.size();
            const InflateRun r = inflate_host_append(z, zn, cur * 8, out, m0, true);
            if (r.status != kInfFinal && r.status != kInfFlush) return fail(c, SNAPHASH_EFORMAT, "gzip: corrupt DEFLATE stream");
            st.segments++;
            st.host_bytes += out.size() - o0;
            if (int e = ds.mirror(o0, out.size())) return e;
            if (r.status == kInfFinal) { ended = true; final_bit = r.end_bit; }
            else cur = r.end_bit >> 3;
            return 0;
        };
        if (split && zn >= kSplitMinBytes) { // block mode: the whole member
            rc = gunzip_blocks(x, c, z, zn, ds, m0, st, kms, &final_bit);
            if (rc) return rc;
            ended = true;
        }
        while (!ended) {
            // the default configuration decodes the segments on host threads (measured faster than the kernel:
            // DESIGN.md sec. 14); SNAPHASH_FLAG_GPU_ONLY sends every linked segment through the kernel
            const uint64_t pn = std::min<uint64_t>(host_mode ? kHostPiece : P, zn - cur);
            std::vector<uint32_t> cand;
            if (host_mode) {
                for (uint64_t v : flush_candidates(z + cur, pn)) cand.push_back((uint32_t)v);
            } else {
                HIP_TRY(c, hipMemcpyAsync(c->inf.d_in.data(), z + cur, pn, hipMemcpyHostToDevice, c->f_stream));
                HIP_TRY(c, hipMemsetAsync(c->inf.d_cand.data(), 0, 4, c->f_stream));
                Span ev;
                if (int erc = span_begin(c, Ev::Codec, c->f_stream, &ev)) return erc;
                HIP_TRY(c, launch_inflate_scan(c->inf.d_in.data(), pn, c->inf.d_cand.data() + 1, c->inf.d_cand.data(), (uint32_t)c->inf.cand_cap(), c->f_stream));
                if (int erc = span_end(c, ev, c->f_stream)) return erc;
                HIP_TRY(c, hipMemcpyAsync(c->inf.h_cand.data(), c->inf.d_cand.data(), 4, hipMemcpyDeviceToHost, c->f_stream));
                HIP_TRY(c, hipStreamSynchronize(c->f_stream));
                kms += span_ms(ev);
                const uint64_t ncand = std::min<uint64_t>(c->inf.h_cand[0], c->inf.cand_cap());
                if (ncand) {
                    HIP_TRY(c, hipMemcpyAsync(c->inf.h_cand.data() + 1, c->inf.d_cand.data() + 1, ncand * 4, hipMemcpyDeviceToHost, c->f_stream));
                    HIP_TRY(c, hipStreamSynchronize(c->f_stream));
                }
                cand.assign(c->inf.h_cand.data() + 1, c->inf.h_cand.data() + 1 + ncand);
            }
            // candidate starts in order, the piece's own start first (past the launch's slots the piece is cut)
            cand.push_back(0);
            std::sort(cand.begin(), cand.end());
            cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
            if (cand.size() > (host_mode ? std::min<uint32_t>(slots, 512) : slots)) cand.resize(host_mode ? std::min<uint32_t>(slots, 512) : slots);
            if (cand.size() == 1 && pn == zn - cur) { // no flush point ahead: the host's stretch
                rc = host_run();
                if (rc) return rc;
                continue;
            }
            const uint32_t K = (uint32_t)cand.size();
            if (host_mode) {
                // the kernel's work on host threads: every candidate decoded speculatively into a slot by the workers, in
                // order, while this thread links the chain and fills each linked segment's holes as soon as it is decoded
                // (in chain order: the bytes in front of a segment are final when it is filled)
                hslots.resize((size_t)K * kInflateSlotSyms);
                hbytes.resize((size_t)K * kInflateSlotSyms);
                std::unique_ptr<std::atomic<uint32_t>[]> done(new std::atomic<uint32_t>[K]);
                for (uint32_t i = 0; i < K; ++i) done[i].store(0, std::memory_order_relaxed);
                std::atomic<uint32_t> next{0};
                auto work = [&]() {
                    InflateTables t;
                    for (;;) {
                        const uint32_t i = next.fetch_add(1);
                        if (i >= K) return;
                        const InflateRun r = inflate_run<uint16_t>(z + cur, pn, (uint64_t)cand[i] * 8, hslots.data() + (size_t)i * kInflateSlotSyms,
                                                                   0, kInflateSlotSyms, true, true, t);
                        // the bytes that are no holes, narrowed here in parallel; the holes are left to the linking thread
                        const uint16_t* sy = hslots.data() + (size_t)i * kInflateSlotSyms;
                        uint8_t* by = hbytes.data() + (size_t)i * kInflateSlotSyms;
                        uint32_t last = 0;
                        for (uint32_t q = 0; q < (uint32_t)r.out_len; ++q) {
                            by[q] = (uint8_t)sy[q];
                            last = sy[q] >= kInfHole ? q + 1 : last;
                        }
                        c->inf.h_res[i] = InflateSegRes{r.end_bit, (uint32_t)r.out_len, last, r.status, 0};
                        done[i].store(1, std::memory_order_release);
                    }
                };
                const unsigned T = (unsigned)std::min<uint64_t>(K, std::max(2u, call_cpus(x)) - 1);
                ThreadJoiner th;
                for (unsigned k = 0; k < T; ++k) th.spawn(work);
                const size_t o0 = out.size();
                uint64_t pos = 0;
                uint32_t nl = 0;
                bool fin = false, bad = false;
                for (;;) {
                    const auto it = std::lower_bound(cand.begin(), cand.end(), (uint32_t)pos);
                    if (it == cand.end() || *it != pos) break;
                    const uint32_t i = (uint32_t)(it - cand.begin());
                    while (!done[i].load(std::memory_order_acquire)) std::this_thread::yield();
                    const InflateSegRes& r = c->inf.h_res[i];
                    if (r.status != kInfFlush && r.status != kInfFinal) break;
                    const size_t base = out.size();
                    out.resize(base + r.out_len);
                    memcpy(out.data() + base, hbytes.data() + (size_t)i * kInflateSlotSyms, r.out_len);
                    if (!fill_holes_host(hslots.data() + (size_t)i * kInflateSlotSyms, r.hole_end, out.data() + base, base - m0)) { bad = true; break; }
                    ++nl;
                    if (r.status == kInfFinal) { fin = true; final_bit = r.end_bit + cur * 8; break; }
                    pos = r.end_bit >> 3;
                    if (pos >= pn) break;
                }
                next.store(K); // (what is left of the piece is decoded again as the next piece)
                th.join_all();
                if (bad) return fail(c, SNAPHASH_EFORMAT, "gzip: a back-reference before the start of the member");
                if (nl == 0) {
                    rc = host_run();
                    if (rc) return rc;
                    continue;
                }
                rc = ds.mirror(o0, out.size());
                if (rc) return rc;
                st.segments += nl;
                if (fin) ended = true;
                else cur += pos;
                continue;
            } else {
                memcpy(c->inf.h_cand.data() + 1, cand.data(), (size_t)K * 4);
                HIP_TRY(c, hipMemcpyAsync(c->inf.d_cand.data() + 1, c->inf.h_cand.data() + 1, (size_t)K * 4, hipMemcpyHostToDevice, c->f_stream));
                Span ev;
                if (int erc = span_begin(c, Ev::Codec, c->f_stream, &ev)) return erc;
                HIP_TRY(c, launch_inflate_decode(c->inf.d_in.data(), pn, c->inf.d_cand.data() + 1, K, c->inf.d_slots.data(), c->inf.d_res.data(), c->f_stream));
                if (int erc = span_end(c, ev, c->f_stream)) return erc;
                HIP_TRY(c, hipMemcpyAsync(c->inf.h_res.data(), c->inf.d_res.data(), (size_t)K * sizeof(InflateSegRes), hipMemcpyDeviceToHost, c->f_stream));
                HIP_TRY(c, hipStreamSynchronize(c->f_stream));
                kms += span_ms(ev);
            }
            // link: from the piece's start, each segment where the one before ended
            uint32_t nl = 0;
            uint64_t pos = 0, off = 0;
            bool fin = false;
            for (;;) {
                const auto it = std::lower_bound(cand.begin(), cand.end(), (uint32_t)pos);
                if (it == cand.end() || *it != pos) break;
                const uint32_t i = (uint32_t)(it - cand.begin());
                const InflateSegRes& r = c->inf.h_res[i];
                if (r.status != kInfFlush && r.status != kInfFinal) break;
                InflateLink& L = c->inf.h_links[nl++];
                L.off = off;
                L.slot = i;
                L.len = r.out_len;
                L.hole_end = r.hole_end;
                L.pad = 0;
                off += r.out_len;
                if (r.status == kInfFinal) { fin = true; final_bit = r.end_bit + cur * 8; break; }
                pos = r.end_bit >> 3;
                if (pos >= pn) break;
            }
            if (trace) {
                const auto it = std::lower_bound(cand.begin(), cand.end(), (uint32_t)pos);
                const int why = (it == cand.end() || *it != pos) ? -1 : c->inf.h_res[it - cand.begin()].status;
                fprintf(stderr, "snaphash inflate: piece at %llu, %llu bytes, %u candidates, chain of %u, stopped at %llu (%d)\n",
                        (unsigned long long)cur, (unsigned long long)pn, K, nl, (unsigned long long)pos, fin ? 100 : why);
            }
            if (nl == 0) { // the segment at the piece's start is not the kernel's (too long for a slot, or a gap): the host's
                rc = host_run();
                if (rc) return rc;
                continue;
            }
            rc = gpu_fill_concat(c, nl, off, kInflateSlotSyms, ds, m0, trace, kms);
            if (rc < 0) return rc;
            if (rc) { // (cannot happen after the ordered sweep; the host decodes the piece's first segment if it does)
                rc = host_run();
                if (rc) return rc;
                continue;
            }
            st.segments += nl;
            st.gpu_segments += nl;
            if (fin) ended = true;
            else cur += pos;
            scratch_spans_done(c);
        }
        scratch_spans_done(c);
        uint32_t crc;
        const size_t tr = (size_t)((final_bit + 7) >> 3);
        if (dev_crc && tr + 8 <= zn) { // the stored value now (the trailer's place and ISIZE are still checked here), the bytes' own below
            crc = z[tr] | (uint32_t)z[tr + 1] << 8 | (uint32_t)z[tr + 2] << 16 | (uint32_t)z[tr + 3] << 24;
            m_off.push_back(m0);
            m_len.push_back(out.size() - m0);
            m_crc.push_back(crc);
        } else {
            crc = crc_parallel(out.data() + m0, out.size() - m0);
            if (tally) tally->host_ranges++;
        }
        size_t next = 0;
        if (gzip_trailer(z, zn, final_bit, crc, out.size() - m0, &next)) return fail(c, SNAPHASH_EFORMAT, "gzip: CRC-32 or ISIZE mismatch");
        at += h + next;
    }
    if (!m_off.empty()) {
        rc = ds.reserve_dev(c, 1, 0); // (every member empty: nothing was written there yet, but the kernel takes a base)
        if (rc) return rc;
        std::vector<uint32_t> got(m_off.size());
        double ms = 0;
        rc = crc_ranges_dev(c, kCrcGzip, c->inf.d_out.data(), m_off.data(), m_len.data(), m_off.size(), got.data(), c->f_stream, &ms);
        scratch_spans_done(c);
        if (rc) return rc;
        if (tally) { tally->device_ranges += m_off.size(); tally->device_ms += ms; }
        if (got != m_crc) return fail(c, SNAPHASH_EFORMAT, "gzip: CRC-32 or ISIZE mismatch");
    }
    st.inflate_ms += kms;
    return SNAPHASH_OK;
}

const UnpackCodec kGunzipCodec = {"gzip", gunzip_engine};

// ---- the tar side: archive/tar's reader as UnpackTar drives it ---------------------------------------------------------

// (TarEntry, go_clean, tar_read and last_regular_members: tar_core.h)
static_assert(kTarEFormat == SNAPHASH_EFORMAT && kTarEContent == SNAPHASH_ECONTENT, "tar_core.h restates the two codes");

int mkdir_all(const std::string& dir)
{
    struct stat s;
    if (stat(dir.c_str(), &s) == 0) return S_ISDIR(s.st_mode) ? 0 : ENOTDIR;
    const size_t sl = dir.find_last_of('/');
    if (sl != std::string::npos && sl > 0) {
        const int e = mkdir_all(dir.substr(0, sl));
        if (e) return e;
    }
    if (mkdir(dir.c_str(), 0777) != 0 && errno != EEXIST) return errno;
    return 0;
}

// UnpackTar's loop: the members of the decoded stream into target (helpers.go:106-142)
int unpack_members(DevCtx* c, const std::vector<TarEntry>& ents, const uint8_t* tar, const std::string& target)
{
    for (const TarEntry& e : ents) {
        const std::string path = go_clean(target + "/" + e.name);
        const size_t sl = path.find_last_of('/');
        const std::string dir = sl == std::string::npos ? "." : (sl == 0 ? "/" : path.substr(0, sl));
        if (int er = mkdir_all(dir)) return fail(c, SNAPHASH_EIO, dir + ": " + strerror(er));
        if (e.type == '5') {
            (void)mkdir(path.c_str(), e.mode); // (an error here is ignored, as in the reference)
        } else if (e.type == '2') {
            if (symlink(e.linkname.c_str(), path.c_str()) != 0) return fail(c, SNAPHASH_EIO, path + ": " + strerror(errno));
        } else {
            const int fd = open(path.c_str(), O_WRONLY | O_TRUNC | O_CREAT | O_CLOEXEC, e.mode);
            if (fd < 0) return fail(c, SNAPHASH_EIO, path + ": " + strerror(errno));
            uint64_t off = 0;
            while (off < e.size) {
                const ssize_t w = write(fd, tar + e.data_off + off, (size_t)std::min<uint64_t>(e.size - off, 1u << 30));
                if (w < 0) {
                    if (errno == EINTR) continue;
                    const int er = errno;
                    close(fd);
                    return fail(c, SNAPHASH_EIO, path + ": " + strerror(er));
                }
                off += (uint64_t)w;
            }
            if (close(fd) != 0) return fail(c, SNAPHASH_EIO, path + ": " + strerror(errno));
        }
    }
    return SNAPHASH_OK;
}

// a whole file into memory, in one pass
int read_whole(snaphash_ctx* x, const char* path, std::vector<uint8_t>& gz)
{
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return fail(x, SNAPHASH_EIO, std::string(path) + ": " + strerror(errno));
    struct stat sb;
    if (fstat(fd, &sb) != 0) { const int er = errno; close(fd); return fail(x, SNAPHASH_EIO, strerror(er)); }
    gz.resize((size_t)sb.st_size);
    size_t got = 0;
    while (got < gz.size()) {
        const ssize_t r = pread(fd, gz.data() + got, gz.size() - got, (off_t)got);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) { const int er = r < 0 ? errno : EIO; close(fd); return fail(x, SNAPHASH_EIO, std::string(path) + ": " + strerror(er)); }
        got += (size_t)r;
    }
    close(fd);
    return SNAPHASH_OK;
}

// The digests of the regular members reg (indices into ents, ascending) out of the decoded stream, 64 bytes each into
// dig: long members on host threads out of tar, as the producer plans them (targz.inc), the others by the SHA-512 kernels
// out of c->inf.d_out, which holds the same stream; SNAPHASH_FLAG_GPU_ONLY: all on the kernels.
int hash_members(snaphash_ctx* x, DevCtx* c, const std::vector<uint8_t>& tar, const std::vector<TarEntry>& ents, const std::vector<size_t>& reg,
                 std::vector<uint8_t>& dig)
{
    int rc = 0;
    for (const size_t k : reg) // tar_read's promise (tar_core.h), held again here: the kernels read d_out with no check of their own
        if (ents[k].data_off > tar.size() || ents[k].size > tar.size() - ents[k].data_off) return fail(x, SNAPHASH_EFORMAT, "tar: member outside the stream");
    dig.assign(reg.size() * 64 + 64, 0);
    std::vector<uint8_t> on_host(reg.size(), 0);
    MemberHashers mh;
    std::vector<size_t> hosted;
    if (!x->gpu_only && !reg.empty()) {
        const unsigned cpus = call_cpus(x);
        const double pass_s = std::max(0.008, (double)tar.size() / 4.5e9);
        const uint64_t long_from = cpus >= 8 ? 0 : (uint64_t)(44e6 * pass_s);
        std::vector<uint64_t> sizes;
        for (size_t q = 0; q < reg.size(); ++q)
            if (long_from == 0 || ents[reg[q]].size > long_from) { on_host[q] = 1; hosted.push_back(q); sizes.push_back(ents[reg[q]].size); }
        if (!hosted.empty()) {
            mh.start(sizes, std::max(1u, std::min(6u, cpus / 3u)));
            std::vector<MemberHashers::Task> ts;
            for (size_t h = 0; h < hosted.size(); ++h) {
                const TarEntry& e = ents[reg[hosted[h]]];
                ts.push_back(MemberHashers::Task{(uint32_t)h, tar.data() + e.data_off, e.size, true, true, 0});
            }
            mh.give_all(ts);
        }
    }
    std::vector<uint64_t> offs, lens;
    std::vector<size_t> dev_q;
    for (size_t q = 0; q < reg.size(); ++q)
        if (!on_host[q]) { offs.push_back(ents[reg[q]].data_off); lens.push_back(ents[reg[q]].size); dev_q.push_back(q); }
    if (!dev_q.empty()) {
        DevBuf<uint8_t> d_dig;
        HIP_TRY(c, d_dig.reserve(dev_q.size() * 64));
        rc = snaphash_sha512_device(x, c->inf.d_out.data(), offs.data(), lens.data(), dev_q.size(), d_dig.data());
        if (!rc) rc = snaphash_sync(x);
        std::vector<uint8_t> hd(dev_q.size() * 64);
        if (!rc && hipMemcpy(hd.data(), d_dig.data(), hd.size(), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(x, SNAPHASH_EDEVICE, "D2H of digests failed");
        if (rc) return rc;
        for (size_t k = 0; k < dev_q.size(); ++k) memcpy(dig.data() + 64 * dev_q[k], hd.data() + 64 * k, 64);
    }
    if (!hosted.empty()) {
        mh.wait_all();
        mh.stop();
        for (size_t h = 0; h < hosted.size(); ++h) memcpy(dig.data() + 64 * hosted[h], mh.digests.data() + 64 * h, 64);
    }
    return SNAPHASH_OK;
}

// the SHA-512 of p[0..n) on a host core of its own, beside what its scope does; joined where the scope ends at the latest
struct DigestThread {
    std::thread th;
    DigestThread(const uint8_t* p, size_t n, uint8_t* dig)
        : th([=] {
              HostSha s;
              host_sha512_init(s);
              host_sha512_update(s, p, n);
              host_sha512_final(s, dig);
          })
    {
    }
    void join() { if (th.joinable()) th.join(); }
    ~DigestThread() { join(); }
};

// Verify after the members were written: the regular members' digests out of the decoded stream tar (which c->inf.d_out
// holds too), then Verify's own comparison on the unpacked tree (its walk is Lstat only: the modes as they are on disk); a
// record whose bytes came from the archive takes their digest, anything else there was before is hashed from disk.
int verify_unpacked(snaphash_ctx* x, DevCtx* c, const std::vector<uint8_t>& tar, const std::vector<TarEntry>& ents, const char* target_dir,
                    const char* archive, const uint8_t* adig, const char* yaml, size_t yaml_len, snaphash_mismatch* first)
{
    const std::vector<size_t> reg = last_regular_members(ents); // members hashed: the last member of a name is what is on disk
    std::vector<uint8_t> dig;
    const int rc = hash_members(x, c, tar, ents, reg, dig);
    if (rc) return rc;
    std::unordered_map<std::string, size_t> dig_of;
    for (size_t q = 0; q < reg.size(); ++q) dig_of[ents[reg[q]].name] = q;
    return verify_impl(x, target_dir, archive, adig, yaml, yaml_len, first, [&](const Record& r, uint8_t* d) {
        const auto it = dig_of.find(r.name);
        if (it == dig_of.end() || (int64_t)ents[reg[it->second]].size != r.size) return false;
        memcpy(d, dig.data() + 64 * it->second, 64);
        return true;
    });
}

// ClickDeb.Unpack after the choice of decoder, for every data-member format: the archive read once, its digest on a host
// core beside the decode, the codec's decoder into the tar stream (kept in c->inf.d_out too when hashes.yaml asks for
// Verify), then tar_read, unpack_members and verify_unpacked.  The body of the snaphash_tar_unpack* entry points.
int tar_unpack_entry(snaphash_ctx* x, const UnpackCodec& codec, const char* archive, const char* target_dir, const char* yaml, size_t yaml_len,
                     snaphash_mismatch* first, uint8_t* archive_digest)
try {
    if (!x || !archive || !target_dir) return fail(x, SNAPHASH_EINVAL, "bad argument");
    TOP_ENTER(x);
    DevCtx* c = x->d0();
    HIP_TRY(c, hipSetDevice(c->device));
    snaphash_unpack_stats st{};
    st.struct_size = sizeof st;
    // the archive, read once
    std::vector<uint8_t> gz; // (the compressed archive)
    int rd = read_whole(x, archive, gz);
    if (rd) return rd;
    st.gz_bytes = gz.size();
    // the archive digest over the compressed bytes, on a host core beside the decode
    uint8_t adig[64];
    DigestThread dig_th(gz.data(), gz.size(), adig);
    std::vector<uint8_t> tar;
    const bool want_verify = yaml != nullptr;
    DecodedStream ds(c, tar, want_verify);
    int rc = codec.decode(x, c, gz.data(), gz.size(), ds, st, CrcAt::Host, nullptr);
    scratch_spans_done(c);
    st.tar_bytes = tar.size();
    std::vector<TarEntry> ents;
    std::string why;
    if (!rc) {
        rc = tar_read(tar.data(), tar.size(), ents, why);
        if (rc) rc = fail(c, rc, why);
    }
    st.members = ents.size();
    if (!rc) rc = unpack_members(c, ents, tar.data(), target_dir);
    dig_th.join();
    if (archive_digest) memcpy(archive_digest, adig, 64);
    if (rc) rc = lift(x, c, rc);
    else if (want_verify) rc = verify_unpacked(x, c, tar, ents, target_dir, archive, adig, yaml, yaml_len, first);
    st.wall_ms = now_ms() - t_top0_;
    x->unpack = st;
    end_top(x, t_top0_);
    return rc;
} catch (...) { // allocation or thread-creation failure: no C++ exception crosses the C boundary
    return SNAPHASH_ENOMEM;
}

// A whole compressed buffer decoded into memory the caller frees: the body of the snaphash_*_buffer entry points.
int decode_to_malloc(snaphash_ctx* x, const UnpackCodec& codec, const void* in, size_t n, void** out, size_t* out_len)
try {
    if (!x || (!in && n) || !out || !out_len) return fail(x, SNAPHASH_EINVAL, "bad argument");
    *out = nullptr;
    *out_len = 0;
    TOP_ENTER(x);
    DevCtx* c = x->d0();
    HIP_TRY(c, hipSetDevice(c->device));
    snaphash_unpack_stats st{};
    st.struct_size = sizeof st;
    st.gz_bytes = n;
    std::vector<uint8_t> o;
    DecodedStream ds(c, o, false);
    const int rc = codec.decode(x, c, (const uint8_t*)in, n, ds, st, CrcAt::Host, nullptr);
    scratch_spans_done(c);
    st.tar_bytes = o.size();
    st.wall_ms = now_ms() - t_top0_;
    x->unpack = st;
    end_top(x, t_top0_);
    if (rc) return lift(x, c, rc);
    void* p = malloc(o.size() ? o.size() : 1);
    if (!p) return fail(x, SNAPHASH_ENOMEM, "malloc");
    if (!o.empty()) memcpy(p, o.data(), o.size());
    *out = p;
    *out_len = o.size();
    return SNAPHASH_OK;
} catch (...) { // allocation or thread-creation failure: no C++ exception crosses the C boundary
    return SNAPHASH_ENOMEM;
}

} // namespace

extern "C" {

int snaphash_gunzip_buffer(snaphash_ctx* x, const void* gz, size_t n, void** out, size_t* out_len)
{
    return decode_to_malloc(x, kGunzipCodec, gz, n, out, out_len);
}

int snaphash_tar_unpack(snaphash_ctx* x, const char* data_tar_gz, const char* target_dir, const char* yaml, size_t yaml_len,
                        snaphash_mismatch* first, uint8_t* archive_digest)
{
    return tar_unpack_entry(x, kGunzipCodec, data_tar_gz, target_dir, yaml, yaml_len, first, archive_digest);
}

int snaphash_get_unpack_stats(const snaphash_ctx* x, snaphash_unpack_stats* out)
{
    if (!x || !out || out->struct_size < sizeof(snaphash_unpack_stats)) return SNAPHASH_EINVAL;
    *out = x->unpack;
    out->struct_size = sizeof(snaphash_unpack_stats);
    return SNAPHASH_OK;
}

int snaphash_get_block_scan_stats(const snaphash_ctx* x, snaphash_block_scan_stats* out)
{
    if (!x || !out || out->struct_size < sizeof(snaphash_block_scan_stats)) return SNAPHASH_EINVAL;
    *out = x->block_scan;
    out->struct_size = sizeof(snaphash_block_scan_stats);
    return SNAPHASH_OK;
}

} // extern "C"
