// targz.inc -- the data.tar.gz producer (SURVEY sec. 8 rows f3 + f2), textually part of
// snaphash_api.cpp (it uses the engine's staging slots and job launcher).
//
// tarCreate (reference clickdeb/deb.go:261-344) walks the tree, streams every file into a tar
// writer wrapped in gzip level 9; Build's callback then hashes the archive and reads every file
// a second time for hashes.yaml (snappy/build.go:216-270).  Here ONE pass does all three: the tar
// stream is assembled in the pinned staging slot (parallel pread of file contents at their tar
// offsets), copied to HBM once, and there (a) the block-parallel DEFLATE kernel compresses it and
// (b) the SHA-512 kernels hash every regular file straight out of the staged tar stream (its
// content starts on a 512-byte boundary).  The compressed bytes come back, are appended to the
// .gz and feed the archive digest -- one sequential stream, hashed on a host core by the
// library's own SHA-512 (a lone stream is 10x faster there than on the GPU).
//
// The file also holds what the three build-side formats share: OutPipe (the consumers), Encoder (a format's parameters and
// running state, made for one call: GzipEncoder here, XzEncoder in xzpack.inc, BzEncoder in bzpack.inc), tar_create_impl (the
// pass, which takes an Encoder) and encode_to_malloc (the body of the *_buffer entries).  Where a slot's headers, padding
// and members' bytes lie is tarpack.cpp's tar_fill_slot, host code with a CPU suite of its own (tests/test_f3_host.py).

namespace {

#define HIP_TRY_BREAK(expr)                                                                              \
    {                                                                                                \
        const hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                      \
            rc = fail(c, SNAPHASH_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));       \
            break;                                                                                   \
        }                                                                                            \
    }

// One piece of output on its way to the consumers.  buf >= 0: the bytes lie in the pinned buffer z.h_out[buf], which
// the producer reuses once every consumer has let go of it; buf < 0: a small piece the item owns.
struct GzItem {
    const uint8_t* p = nullptr;
    size_t n = 0;
    int buf = -1;
    std::shared_ptr<std::vector<uint8_t>> own;
};

// The gzip producer's self-check, asked for by snaphash_snap_build alone: every piece's compacted bytes are walked against
// the staged stream by deflate_check_kernel before they leave HBM (deflate_check_core.h).
struct GzCheck {
    const char* member = ""; // for last_error
    uint64_t chunks = 0;     // chunks checked (all accepted, or the call failed)
    double ms = 0;           // the check kernel's own time, HIP events
};

// What every compressor hands its bytes to (gz_emit): the pass's two consumers, or a string in memory.
struct OutPipe {
    DevCtx* c = nullptr;
    int fd = -1;                 // output file, or -1: collect into `mem`
    std::string* mem = nullptr;
    uint64_t out_bytes = 0;
    // Two consumers take the compressed bytes in order, off the producer's thread: one appends them to the file,
    // one absorbs them into the archive digest (the stream that cannot be parallel: it bounds the whole pass).
    bool want_sha = false;
    HostSha sha;
    std::thread sha_thread, wr_thread;
    std::mutex mu;
    std::condition_variable cv;
    std::queue<GzItem> q_sha, q_wr;
    int inflight[2] = {0, 0};    // consumers still reading the encoder's pinned output buffer b
    int write_err = 0;
    bool closing = false;
    double busy_ms[2] = {0, 0}, wait_ms[2] = {0, 0}; // per consumer (digest, writer): working / waiting for the producer
    double t_first_piece = 0, t_last_piece = 0;      // when the compressor's first / last piece went to the consumers (trace)
    snaphash_targz_stats st{};
    // Whatever way the producer leaves (an exception on its way to the C boundary's catch included), the consumers are
    // told to finish and are joined: a joinable std::thread that is destroyed takes the process down.
    ~OutPipe()
    {
        { std::lock_guard<std::mutex> lk(mu); closing = true; }
        cv.notify_all();
        if (sha_thread.joinable()) sha_thread.join();
        if (wr_thread.joinable()) wr_thread.join();
    }
};

// What tar_create_impl and encode_to_malloc ask of a compressor (tarCreate's switch on the suffix, deb.go:269-276): the gzip
// encoder below, the .xz encoder in xzpack.inc, the .bz2 encoder in bzpack.inc.  An encoder is made for one call, with the
// call's parameters, and holds the stream's running state; all hand their bytes to the consumers through gz_emit.
struct GzipEncoder;
struct Encoder {
    const char* const suffix;
    const char* const staging_refusal;  // encode_to_malloc's words when a slot outgrows the engine's staging size; null: none does
    GzipEncoder* parts = nullptr;       // set: the pass's first slot may be compressed while it is still being filled (gz_slot_begin / _launch / _consume)
    double* check_ms = nullptr;         // where the time of the call's events of kind 3 goes (the gzip self-check's kernel); null: there are none
    Encoder(const char* sfx, const char* refusal) : suffix(sfx), staging_refusal(refusal) {}
    virtual ~Encoder() = default;
    virtual uint64_t slot_bytes(const DevCtx* c, uint64_t job_bytes) const = 0; // what the pass stages at a time (a multiple of 512)
    virtual int ensure(DevCtx* c, uint64_t slot_bytes) = 0;
    virtual void begin(OutPipe& g) = 0;                                         // what the file begins with
    virtual int slot(OutPipe& g, Slot& sl, uint64_t n, hipEvent_t ready, int zbuf, bool is_first, bool is_last) = 0;
    virtual int finish(OutPipe& g, uint8_t archive_digest[64]) = 0;             // what it ends with; -> errno of the first failed write, or 0
};

struct GzipEncoder final : Encoder {
    uint32_t crc = 0;            // of the uncompressed stream
    uint64_t isize = 0;
    // the slot in the compressor (gz_slot_begin / _launch / _consume)
    std::vector<std::pair<uint32_t, uint32_t>> z_pieces; // (first chunk, count)
    uint32_t z_nch = 0, z_launched = 0;
    Span z_evpair{};
    // the self-check (snapbuild.inc, SNAPHASH_BUILD_CHECK): null = off, the compressor's path without it
    GzCheck* const check;
    explicit GzipEncoder(GzCheck* chk = nullptr) : Encoder(".gz", nullptr), check(chk)
    {
        parts = this;
        if (chk) check_ms = &chk->ms;
    }
    uint64_t slot_bytes(const DevCtx* c, uint64_t job_bytes) const override;
    int ensure(DevCtx* c, uint64_t slot_bytes) override;
    void begin(OutPipe& g) override;
    int slot(OutPipe& g, Slot& sl, uint64_t n, hipEvent_t ready, int zbuf, bool is_first, bool is_last) override;
    int finish(OutPipe& g, uint8_t archive_digest[64]) override;
};

// What a call of the producer stages at a time: the engine's staging size, or -- for a job smaller than that -- the next
// power of two that holds it (at least 8 MiB).  The staging slots and the compressor's buffers are sized for it and grow when
// a later call needs more.  (Round 5: one `snaphash build` of a 20 MiB package spent 240 of its 270 ms pinning 2 x 256 MiB of
// staging and 2 x 256 MiB of output buffers it would never fill: tools/cli_latency_probe.sh.)
uint64_t producer_slot_bytes(const DevCtx* c, uint64_t job_bytes)
{
    const uint64_t full = std::max<uint64_t>(c->staging & ~(uint64_t)(kDeflateChunk - 1), kDeflateChunk);
    uint64_t want = 8u << 20;
    while (want < job_bytes && want < full) want <<= 1;
    want = std::min(want, full);
    // (larger staging slots that another call left behind are used in part: the compressor's own buffers are sized by this too,
    // and a small package in a ctx that has hashed a big tree should not pin them at that tree's size)
    return std::max<uint64_t>(want & ~(uint64_t)(kDeflateChunk - 1), kDeflateChunk);
}

// the two streams every encoder works on
int ensure_producer_streams(DevCtx* c)
{
    if (!c->z_stream) { // the compressor's own stream, below the hashing kernels in priority: they are the longer chain
        int least = 0, greatest = 0;
        HIP_TRY(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_TRY(c, c->z_stream.ensure(hipStreamNonBlocking, least));
    }
    HIP_TRY(c, c->z2_stream.ensure(hipStreamNonBlocking)); // concatenation + the way back
    return SNAPHASH_OK;
}

uint64_t GzipEncoder::slot_bytes(const DevCtx* c, uint64_t job_bytes) const { return producer_slot_bytes(c, job_bytes); }

int GzipEncoder::ensure(DevCtx* c, uint64_t slot_bytes)
{
    const size_t nch = (size_t)((slot_bytes + kDeflateChunk - 1) / kDeflateChunk);
    const int rc = ensure_producer_streams(c);
    if (rc) return rc;
    // (grown: what a smaller job left behind goes first; a failure leaves none of it, and the next call allocates it all)
    HIP_TRY(c, c->z.ensure(nch, c->numa_node));
    if (check) HIP_TRY(c, c->z.chk.ensure(nch));
    return SNAPHASH_OK;
}

// buf >= 0: p points into z.h_out[buf] (stays valid until gz_wait_buf(buf) returns); buf < 0: p is copied.
void gz_emit(OutPipe& g, const uint8_t* p, size_t n, int buf)
{
    if (n == 0) return;
    if (g.mem) g.mem->append((const char*)p, n);
    g.out_bytes += n;
    if (buf >= 0) { g.t_last_piece = now_ms(); if (g.t_first_piece == 0) g.t_first_piece = g.t_last_piece; }
    if (g.fd < 0 && !g.want_sha) return;
    GzItem it;
    it.n = n;
    it.buf = buf;
    if (buf < 0) {
        it.own = std::make_shared<std::vector<uint8_t>>(p, p + n);
        it.p = it.own->data();
    } else {
        it.p = p;
    }
    std::lock_guard<std::mutex> lk(g.mu);
    if (g.fd >= 0) { g.q_wr.push(it); if (buf >= 0) g.inflight[buf]++; }
    if (g.want_sha) { g.q_sha.push(it); if (buf >= 0) g.inflight[buf]++; }
    g.cv.notify_all();
}

void gz_wait_buf(OutPipe& g, int buf)
{
    std::unique_lock<std::mutex> lk(g.mu);
    g.cv.wait(lk, [&] { return g.inflight[buf] == 0; });
}

void gz_consumer(OutPipe* g, bool is_writer)
{
    std::queue<GzItem>& q = is_writer ? g->q_wr : g->q_sha;
    for (;;) {
        GzItem it;
        const double tw0 = now_ms();
        {
            std::unique_lock<std::mutex> lk(g->mu);
            g->cv.wait(lk, [&] { return !q.empty() || g->closing; });
            if (q.empty()) return;
            it = std::move(q.front());
            q.pop();
        }
        const double tb0 = now_ms();
        g->wait_ms[is_writer] += tb0 - tw0;
        if (is_writer) {
            size_t off = 0;
            int err = 0;
            while (off < it.n) {
                const ssize_t w = write(g->fd, it.p + off, it.n - off);
                if (w < 0) { if (errno == EINTR) continue; err = errno; break; }
                off += (size_t)w;
            }
            if (err) { std::lock_guard<std::mutex> lk(g->mu); if (!g->write_err) g->write_err = err; }
        } else {
            host_sha512_update(g->sha, it.p, it.n);
        }
        g->busy_ms[is_writer] += now_ms() - tb0;
        if (it.buf >= 0) {
            std::lock_guard<std::mutex> lk(g->mu);
            g->inflight[it.buf]--;
            g->cv.notify_all();
        }
    }
}

void gz_begin(OutPipe& g)
{
    if (g.want_sha) {
        host_sha512_init(g.sha);
        g.sha_thread = std::thread(gz_consumer, &g, false);
    }
    if (g.fd >= 0) g.wr_thread = std::thread(gz_consumer, &g, true);
}

// CRC-32 of the staged piece on a few host threads (ranges, then combined in order)
uint32_t crc_parallel(const uint8_t* p, size_t n)
{
    const size_t kRange = 4u << 20;
    const size_t nr = (n + kRange - 1) / kRange;
    if (nr <= 1) return crc32_update(0, p, n);
    std::vector<uint32_t> part(nr);
    std::atomic<size_t> next{0};
    auto work = [&]() {
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= nr) return;
            part[i] = crc32_update(0, p + i * kRange, std::min(kRange, n - i * kRange));
        }
    };
    // four threads at ~8 GB/s each (crc32_clmul) finish a 256 MiB slot inside its first piece's kernel; more would only
    // take cores from the staging fill of the next slot and from the archive digest, the thread that bounds the pass
    const unsigned T = (unsigned)std::min<size_t>(std::min(4u, usable_cpus()), nr);
    ThreadJoiner th;
    for (unsigned t = 1; t < T; ++t) th.spawn(work);
    work();
    th.join_all();
    uint32_t crc = part[0];
    for (size_t i = 1; i < nr; ++i) crc = crc32_combine(crc, part[i], std::min(kRange, n - i * kRange));
    return crc;
}

// A slot's bytes -> deflate chunks -> concatenation -> pinned z.h_out[zbuf] -> the consumers.
// The slot is compressed in pieces of kZPiece chunks: all chunk kernels are enqueued at once on the compressor's
// stream; as each piece's sizes arrive its bytes are concatenated and brought back on a second stream and handed to
// the consumers, while the later pieces are still being compressed -- the archive digest (the stream that bounds the
// pass) starts a piece, not a slot, behind the compressor.
constexpr uint32_t kZPiece = 1024; // (960 / 992 / 2048 chunks a piece measured no better: tools/targz_probe.py) // chunks per piece: 64 MiB, four rounds of 256 workgroups

// pieces of one slot: (first chunk, count).  `first` / `last`: the slot opens / closes the pass.
struct ZPieces {
    uint32_t piece = kZPiece, first = 0, taper = 0;
    ZPieces()
    {
        if (const char* e = getenv("SNAPHASH_ZPIECE")) piece = std::min<uint32_t>(std::max<uint32_t>((uint32_t)strtoul(e, nullptr, 10), 64u), 8192u);
        if (const char* e = getenv("SNAPHASH_ZFIRST")) first = std::min<uint32_t>((uint32_t)strtoul(e, nullptr, 10), 8192u);
        if (const char* e = getenv("SNAPHASH_ZTAPER")) taper = std::min<uint32_t>((uint32_t)strtoul(e, nullptr, 10), 8192u);
    }
    void cut(uint32_t nch, bool is_first, bool is_last, std::vector<std::pair<uint32_t, uint32_t>>& out) const
    {
        out.clear();
        uint32_t c0 = 0;
        if (is_first && first) // a doubling ramp: the consumers start a round, not a piece, behind the compressor and are never left waiting
            for (uint32_t f = first; f < piece && c0 + f < nch; f *= 2u) { out.emplace_back(c0, f); c0 += f; }
        while (c0 < nch) {
            uint32_t cnt = std::min(piece, nch - c0);
            // the pass's last chunks in halving pieces: what is left for the digest after the compressor's last kernel
            if (is_last && taper && nch - c0 <= piece && cnt > taper) cnt = std::min(cnt, std::max(taper, (cnt / 2u + 63u) & ~63u));
            out.emplace_back(c0, cnt);
            c0 += cnt;
        }
    }
};

// One slot on its way through the compressor, in three steps so that the pass's first slot can be compressed while it
// is still being filled: begin (cut into pieces), launch (the pieces whose bytes are in HBM), consume (sizes -> prefix
// -> concatenation -> pinned z.h_out -> the consumers).
int gz_slot_begin(OutPipe& g, GzipEncoder& z, uint64_t n, bool is_first, bool is_last)
{
    DevCtx* c = g.c;
    static const ZPieces zp;
    z.z_nch = (uint32_t)((n + kDeflateChunk - 1) / kDeflateChunk);
    zp.cut(z.z_nch, is_first, is_last, z.z_pieces);
    z.z_launched = 0;
    if (c->z_ev.size() < z.z_pieces.size()) c->z_ev.resize(z.z_pieces.size());
    for (size_t k = 0; k < z.z_pieces.size(); ++k) HIP_TRY(c, c->z_ev[k].ensure(hipEventDisableTiming));
    return span_begin(c, Ev::Codec, c->z_stream, &z.z_evpair); // (ends behind the slot's last piece: gz_slot_launch)
}

// launches, in order, every piece that ends at or before bytes_ready (bytes_ready >= n: all that are left); `ready`
// (may be NULL) is waited for first: the copy that brought those bytes
int gz_slot_launch(OutPipe& g, GzipEncoder& z, Slot& sl, uint64_t n, uint64_t bytes_ready, hipEvent_t ready)
{
    DevCtx* c = g.c;
    hipStream_t zs = c->z_stream;
    bool waited = false;
    while (z.z_launched < z.z_pieces.size()) {
        const uint32_t c0 = z.z_pieces[z.z_launched].first, cnt = z.z_pieces[z.z_launched].second;
        if (bytes_ready < n && (uint64_t)(c0 + cnt) * kDeflateChunk > bytes_ready) break;
        if (ready && !waited) { HIP_TRY(c, hipStreamWaitEvent(zs, ready, 0)); waited = true; }
        const hipError_t e = launch_deflate_chunks(sl.d_buf.data(), n, c->z.d_slots.data(), c->z.d_sizes.data(), c->z.d_toks.data(), c0, cnt, z.z_nch, c->n_xcd, c->deflate_depth, zs);
        if (e != hipSuccess) return fail(c, SNAPHASH_EDEVICE, std::string("deflate launch: ") + hipGetErrorString(e));
        HIP_TRY(c, hipMemcpyAsync(c->z.h_sizes.data() + c0, c->z.d_sizes.data() + c0, (size_t)cnt * 4, hipMemcpyDeviceToHost, zs));
        HIP_TRY(c, hipEventRecord(c->z_ev[z.z_launched], zs));
        if (++z.z_launched == z.z_pieces.size()) return span_end(c, z.z_evpair, zs);
    }
    return SNAPHASH_OK;
}

int gz_slot_consume(OutPipe& g, GzipEncoder& z, Slot& sl, uint64_t n, int zbuf)
{
    DevCtx* c = g.c;
    hipStream_t zs = c->z_stream, z2 = c->z2_stream;
    if (z.z_launched != z.z_pieces.size()) return fail(c, SNAPHASH_EDEVICE, "a piece of the slot was never launched");
    // while the kernels run: CRC of the uncompressed bytes on a few host threads of their own -- NOT on this thread, which
    // has the pieces to hand on
    struct CrcJob { // joined on every way out
        std::future<uint32_t> f;
        ~CrcJob() { if (f.valid()) f.wait(); }
    } crc_job{std::async(std::launch::async, crc_parallel, (const uint8_t*)sl.h_buf.data(), (size_t)n)};
    gz_wait_buf(g, zbuf); // the consumers have let go of what this buffer held two slots ago
    uint64_t total = 0;
    for (uint32_t k = 0; k < z.z_pieces.size(); ++k) {
        const uint32_t c0 = z.z_pieces[k].first, cnt = z.z_pieces[k].second;
        HIP_TRY(c, hipEventSynchronize(c->z_ev[k]));
        const uint64_t base = total;
        for (uint32_t i = c0; i < c0 + cnt; ++i) {
            c->z.h_prefix[i] = total;
            if (c->z.h_sizes[i] > kDeflateSlot) return fail(c, SNAPHASH_EDEVICE, "deflate kernel reported an impossible chunk size");
            if (c->z.h_sizes[i] == deflate_stored_size((uint32_t)std::min<uint64_t>(kDeflateChunk, n - (uint64_t)i * kDeflateChunk))) g.st.stored_chunks++;
            total += c->z.h_sizes[i];
        }
        HIP_TRY(c, hipMemcpyAsync(c->z.d_prefix.data() + c0, c->z.h_prefix.data() + c0, (size_t)cnt * 8, hipMemcpyHostToDevice, z2));
        Span ev2, ev3;
        if (int rc = span_begin(c, Ev::Codec, z2, &ev2)) return rc;
        const hipError_t e = launch_deflate_compact(c->z.d_slots.data(), c->z.d_sizes.data(), c->z.d_prefix.data(), c->z.d_out.data(), c0, cnt, z2);
        if (e != hipSuccess) return fail(c, SNAPHASH_EDEVICE, std::string("compact launch: ") + hipGetErrorString(e));
        if (int rc = span_end(c, ev2, z2)) return rc;
        if (z.check) { // behind the compaction: the piece's stretches of d_out against the slot's staged bytes
            if (int rc = span_begin(c, Ev::Check, z2, &ev3)) return rc;
            const hipError_t ec = launch_deflate_check(sl.d_buf.data(), n, c->z.d_out.data(), total, c->z.d_prefix.data(), c->z.d_sizes.data(), c0, cnt,
                                                       z.z_nch, false, c->z.chk.d.data(), z2);
            if (ec != hipSuccess) return fail(c, SNAPHASH_EDEVICE, std::string("check launch: ") + hipGetErrorString(ec));
            if (int rc = span_end(c, ev3, z2)) return rc;
            HIP_TRY(c, hipMemcpyAsync(c->z.chk.h.data() + c0, c->z.chk.d.data() + c0, (size_t)cnt * sizeof(DfCheckVerdict), hipMemcpyDeviceToHost, z2));
        }
        HIP_TRY(c, hipMemcpyAsync(c->z.h_out[zbuf].data() + base, c->z.d_out.data() + base, total - base, hipMemcpyDeviceToHost, z2));
        HIP_TRY(c, hipStreamSynchronize(z2));
        if (z.check) {
            for (uint32_t i = c0; i < c0 + cnt; ++i) {
                const DfCheckVerdict v = c->z.chk.h[i];
                if (v.status == kDfCheckOk) continue;
                const uint64_t chunk = g.st.chunks + i; // of the member: the slots before this one, then this slot's
                return fail(c, SNAPHASH_EDEVICE, std::string("self-check: ") + z.check->member + ": chunk " + std::to_string(chunk) + " does not decode to the bytes it was made from (status " +
                                                     std::to_string(v.status) + ") at offset " + std::to_string(chunk * kDeflateChunk + v.offset) + " of the tar stream");
            }
            z.check->chunks += cnt;
        }
        gz_emit(g, c->z.h_out[zbuf].data() + base, total - base, zbuf);
    }
    HIP_TRY(c, hipStreamSynchronize(zs));
    const uint32_t crc = crc_job.f.get();
    z.crc = z.isize ? crc32_combine(z.crc, crc, n) : crc;
    z.isize += n;
    g.st.chunks += z.z_nch;
    return SNAPHASH_OK;
}

// The slot's first n bytes (in sl.h_buf.data(), and in sl.d_buf.data() once `ready` has fired; ready == nullptr: already ordered on the
// compressor's stream), all three steps.
int gz_process_slot(OutPipe& g, GzipEncoder& z, Slot& sl, uint64_t n, hipEvent_t ready, int zbuf, bool is_first = false, bool is_last = false)
{
    if (n == 0) return SNAPHASH_OK;
    int rc = gz_slot_begin(g, z, n, is_first, is_last);
    if (!rc) rc = gz_slot_launch(g, z, sl, n, n, ready);
    if (!rc) rc = gz_slot_consume(g, z, sl, n, zbuf);
    return rc;
}

void gz_join(OutPipe& g)
{
    { std::lock_guard<std::mutex> lk(g.mu); g.closing = true; }
    g.cv.notify_all();
    if (g.sha_thread.joinable()) g.sha_thread.join();
    if (g.wr_thread.joinable()) g.wr_thread.join();
}

// What every encoder's finish ends with: the stream's last bytes, the consumers joined, the archive digest.
// -> errno of the first failed write, or 0
int pipe_finish(OutPipe& g, const uint8_t* tail, size_t n, uint8_t archive_digest[64])
{
    gz_emit(g, tail, n, -1);
    gz_join(g);
    if (g.want_sha && archive_digest) host_sha512_final(g.sha, archive_digest);
    return g.write_err;
}

void GzipEncoder::begin(OutPipe& g) { gz_emit(g, kGzipHeader, sizeof kGzipHeader, -1); }

int GzipEncoder::slot(OutPipe& g, Slot& sl, uint64_t n, hipEvent_t ready, int zbuf, bool is_first, bool is_last)
{
    return gz_process_slot(g, *this, sl, n, ready, zbuf, is_first, is_last);
}

int GzipEncoder::finish(OutPipe& g, uint8_t archive_digest[64])
{
    uint8_t tail[10] = {0x03, 0x00}; // final empty fixed-Huffman block (BFINAL=1, BTYPE=01, end-of-block)
    for (int k = 0; k < 4; ++k) tail[2 + k] = (uint8_t)(crc >> (8 * k));
    for (int k = 0; k < 4; ++k) tail[6 + k] = (uint8_t)((uint32_t)isize >> (8 * k));
    const int werr = pipe_finish(g, tail, sizeof tail, archive_digest);
    if (getenv("SNAPHASH_TRACE_TARGZ"))
        fprintf(stderr, "snaphash targz: digest thread busy %.0f ms, starved %.0f ms; writer busy %.0f ms, starved %.0f ms\n", g.busy_ms[0],
                g.wait_ms[0], g.busy_ms[1], g.wait_ms[1]);
    return werr;
}

void gz_abort(OutPipe& g) { gz_join(g); }

// a producer's ledger at the end of its call: every codec's, CRC's and SHA-256's launch is its deflate_ms, the self-check's its own
void collect_producer_events(DevCtx* c, OutPipe& g, const Encoder& enc)
{
    const SpanSums ev = collect_events(c, false);
    g.st.deflate_ms += ev.codec;
    if (enc.check_ms) *enc.check_ms += ev.check;
}

// A whole buffer through an encoder into memory the caller frees: the body of the snaphash_*_buffer entry points of the
// build side, behind their own argument checks (decode_to_malloc is the install side's).
int encode_to_malloc(snaphash_ctx* x, Encoder& enc, const void* data, size_t n, void** out_p, size_t* out_len)
{
    TOP_ENTER(x);
    DevCtx* c = x->d0();
    HIP_TRY(c, hipSetDevice(c->device));
    const uint64_t S = enc.slot_bytes(c, n);
    if (enc.staging_refusal && S > c->staging) return fail(x, SNAPHASH_EINVAL, enc.staging_refusal);
    int rc = ensure_slots(c, 2, S);
    if (!rc) rc = enc.ensure(c, S);
    if (rc) return lift(x, c, rc);
    std::string out;
    OutPipe g;
    g.c = c;
    g.mem = &out;
    gz_begin(g);
    enc.begin(g);
    Slot& sl = c->slot[0];
    const double t0 = now_ms();
    for (uint64_t off = 0; off < n && !rc; off += S) {
        const uint64_t take = std::min<uint64_t>(S, n - off);
        memcpy(sl.h_buf.data(), (const uint8_t*)data + off, take);
        Span ev; // (recorded in the chain below: its failures keep this call's own text)
        if ((rc = span_take(c, Ev::H2d, &ev))) break;
        if (hipEventRecord(ev.a, c->z_stream) != hipSuccess ||
            hipMemcpyAsync(sl.d_buf.data(), sl.h_buf.data(), take, hipMemcpyHostToDevice, c->z_stream) != hipSuccess ||
            hipEventRecord(ev.b, c->z_stream) != hipSuccess) { rc = fail(c, SNAPHASH_EDEVICE, "H2D failed"); break; }
        rc = enc.slot(g, sl, take, nullptr, 0, off == 0, off + take >= n);
    }
    if (!rc && enc.finish(g, nullptr)) rc = fail(c, SNAPHASH_EIO, "write failed");
    if (rc) gz_abort(g);
    (void)hipStreamSynchronize(c->z_stream);
    (void)hipStreamSynchronize(c->z2_stream);
    collect_producer_events(c, g, enc);
    g.st.tar_bytes = n;
    g.st.gz_bytes = out.size();
    g.st.wall_ms = now_ms() - t0;
    x->targz = g.st;
    merge_stats(x);
    end_top(x, t_top0_);
    if (rc) return lift(x, c, rc);
    void* p = malloc(out.size() ? out.size() : 1);
    if (!p) return fail(x, SNAPHASH_ENOMEM, "malloc");
    memcpy(p, out.data(), out.size());
    *out_p = p;
    *out_len = out.size();
    return SNAPHASH_OK;
}

} // namespace

extern "C" {

int snaphash_gzip_buffer(snaphash_ctx* x, const void* data, size_t n, void** gz_out, size_t* gz_len)
try {
    if (!x || (!data && n) || !gz_out || !gz_len) return fail(x, SNAPHASH_EINVAL, "bad argument");
    *gz_out = nullptr;
    *gz_len = 0;
    GzipEncoder enc;
    return encode_to_malloc(x, enc, data, n, gz_out, gz_len);
} catch (...) { // allocation or thread-creation failure: no C++ exception crosses the C boundary
    return SNAPHASH_ENOMEM;
}

int snaphash_deflate_codes_device(snaphash_ctx* x, const void* d_freq, size_t n_tables, uint32_t n_syms, uint32_t max_bits, void* d_lens,
                                  void* d_codes, void* d_rounds)
try {
    if (!x || (n_tables && (!d_freq || !d_lens || !d_codes || !d_rounds)) || n_tables > 0x7fffffffu || n_syms == 0 || n_syms > kDfCodesMaxSyms ||
        max_bits == 0 || max_bits > (uint32_t)kMaxBits || n_syms > (1u << max_bits))
        return fail(x, SNAPHASH_EINVAL, "bad argument");
    TOP_ENTER(x);
    DevCtx* c = x->d0();
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_deflate_codes((const uint32_t*)d_freq, (uint32_t)n_tables, n_syms, max_bits, (uint8_t*)d_lens, (uint32_t*)d_codes,
                                    (uint32_t*)d_rounds, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    x->stats.launches = n_tables ? 1 : 0;
    end_top(x, t_top0_);
    return SNAPHASH_OK;
} catch (...) { // allocation failure: no C++ exception crosses the C boundary
    return SNAPHASH_ENOMEM;
}

static int tar_create_impl(snaphash_ctx* x, Encoder& enc, const char* tarname, const char* source_dir, const char* exclude_prefix,
                           snaphash_keep_fn keep, void* keep_user, char** yaml_out, size_t* yaml_len, uint8_t* archive_digest)
{
    if (!x || !tarname || !source_dir) return fail(x, SNAPHASH_EINVAL, "bad argument");
    if (yaml_out) *yaml_out = nullptr;
    const size_t tl = strlen(tarname);
    const size_t sfx = strlen(enc.suffix);
    if (tl < sfx || strcmp(tarname + tl - sfx, enc.suffix) != 0) // deb.go:270-276: the entry's own suffix (.xz: snaphash_tar_create_xz, .bz2: _bz2)
        return fail(x, SNAPHASH_EINVAL, std::string("unknown compression extension ") + tarname);
    TOP_ENTER(x);
    DevCtx* c = x->d0(); // several engines: the first one (the pass is bound by the serial archive digest, snaphash.h)
    HIP_TRY(c, hipSetDevice(c->device));
    const double t0 = now_ms();

    TarPlan plan;
    int en = 0;
    std::string what;
    std::vector<WalkEntry> ents; // ONE walk serves the archive and hashes.yaml
    if (walk_entries(source_dir, ents, &en, &what)) return fail(x, SNAPHASH_EIO, what + ": " + strerror(en)); // deb.go:286-289
    int rc = tar_plan_entries(ents, exclude_prefix ? exclude_prefix : "", plan, keep, keep_user);
    if (rc) return fail(x, rc, "tar_plan");
    // hashes.yaml out of the same pass: the record list is writeHashes' own view of the walk (it also rejects what
    // tarCreate silently skips: devices, fifos, sockets)
    const bool fused = yaml_out != nullptr;
    std::vector<Record> recs;
    std::vector<uint32_t> stream_of(plan.members.size(), 0xffffffffu); // member -> row of the digest vector
    size_t nstreams = 0;
    if (fused) {
        rc = records_from_entries(ents, recs);
        if (rc) return fail(x, rc, "Unknown file mode");
        size_t k = 0;
        for (const Record& r : recs) {
            if (!name_emittable(r.name)) return fail(x, SNAPHASH_ENAME, "name outside what the YAML emitter restates (yamlscalar.cpp): " + r.name);
            if (k >= plan.members.size() || plan.members[k].name != "./" + r.name)
                return fail(x, SNAPHASH_EINVAL, "the exclude rule must be writeHashes' own (<dir>/DEBIAN) when hashes.yaml is requested");
            if (r.is_regular) stream_of[k] = (uint32_t)nstreams++;
            ++k;
        }
        if (k != plan.members.size()) return fail(x, SNAPHASH_EINVAL, "tree changed during the pass");
    }
    // Which members' digests come from host threads (member_hashers.h).  In the default configuration, with eight cores or
    // more: ALL of them.  Five workers hash 7 GB/s out of the staging buffer, more than the pass moves -- and the members'
    // SHA-512 kernel costs the compressor more than it saves the host: a piece of the DEFLATE kernel is 1 024 one-CU workgroups,
    // exactly four rounds of the chip's 256 CUs, and a hashing workgroup (64 streams, 140 KB of LDS) holds a CU for ~24 ms, so a
    // piece that overlaps one runs FIVE rounds (12.0 ms against 10.0; profiles/r05_deflate_depths.txt).  With the members on host
    // threads the pass of 1 GiB of text takes 198 ms at depth 96 where it took 214 (204 at depth 72).  With fewer cores: only
    // the members whose chain on the GPU would outlast their slot's share of the pass (a lone chain is 44 MB/s there) -- the
    // members' kernels run slot after slot, each as long as ITS longest piece (a 4 MB member in each of two slots: 92 + 92 ms).
    // SNAPHASH_FLAG_GPU_ONLY: every member through the kernels.
    std::vector<uint32_t> hosted_of(plan.members.size(), 0xffffffffu); // member -> id among the hosted ones
    std::vector<uint64_t> hosted_sizes;
    MemberHashers mh;
    if (fused && !x->gpu_only) {
        const unsigned cpus = call_cpus(x);
        // what the pass takes whatever its members are: ~5 GiB/s of tree, and a floor
        const double pass_s = std::max(0.008, (double)plan.total / 4.5e9);
        const uint64_t slot_bytes = enc.slot_bytes(c, plan.total);
        const uint64_t nslots = std::max<uint64_t>(1, (plan.total + slot_bytes - 1) / slot_bytes);
        uint64_t long_from = cpus >= 8 ? 0 : (uint64_t)(44e6 * pass_s / (double)nslots);
        if (const char* e = getenv("SNAPHASH_LONG_FROM")) long_from = strtoull(e, nullptr, 10); // lab: members longer than this on host threads
        for (size_t k = 0; k < plan.members.size(); ++k)
            if (stream_of[k] != 0xffffffffu && (long_from == 0 || (uint64_t)plan.members[k].size > long_from)) {
                hosted_of[k] = (uint32_t)hosted_sizes.size();
                hosted_sizes.push_back((uint64_t)plan.members[k].size);
            }
        unsigned workers = std::max(1u, std::min(6u, cpus / 3u)); // (16 cores: five, 7 GB/s of members -- a tree that compresses to nothing passes at the kernel's 6)
        if (const char* e = getenv("SNAPHASH_MEMBER_HASHERS")) workers = (unsigned)std::min<unsigned long>(std::max<unsigned long>(strtoul(e, nullptr, 10), 1), 64); // lab
        if (!hosted_sizes.empty()) mh.start(hosted_sizes, workers);
    }
    const uint64_t S = enc.slot_bytes(c, plan.total); // a multiple of 512 and of the compressor's chunk
    if (S > c->staging) return fail(x, SNAPHASH_EINVAL, "the engine's staging size is smaller than what the compressor takes at a time");
    rc = ensure_slots(c, 2, S);
    if (!rc) rc = enc.ensure(c, S);
    if (rc) return lift(x, c, rc);
    if (nstreams) HIP_TRY(x, c->hash.ensure(nstreams, true));

    std::vector<Source> srcs(plan.members.size());
    for (size_t k = 0; k < plan.members.size(); ++k) { srcs[k].path = plan.members[k].path.c_str(); srcs[k].len = (uint64_t)plan.members[k].size; }
    for (Slot& sl : c->slot) HIP_TRY(x, sl.jobs.ensure(nstreams));

    const double t_planned = now_ms();
    struct FdGuard { int fd; ~FdGuard() { if (fd >= 0) close(fd); } } fdg{open(tarname, O_WRONLY | O_CREAT | O_CLOEXEC, 0666)}; // os.Create, with the truncation moved to the END of the pass:
    // cutting a previous data.tar.gz down to nothing here frees its pages while the whole pipeline waits (25-30 ms for
    // 250 MiB on tmpfs, an eighth of the pass; SNAPHASH_TRACE_TARGZ), and the writer then allocates them again.  The
    // bytes are written from offset 0 over whatever is there and the length is set when all of them are
    // (ftruncate below); the file is unlinked if the pass fails, as before.
    const int fd = fdg.fd;
    if (fd < 0) return fail(x, SNAPHASH_EIO, std::string(tarname) + ": " + strerror(errno));
    const double t_opened = now_ms();
    double t_first_fill = 0;
    OutPipe g; // declared after the guard: its consumers are joined before the descriptor closes
    g.c = c;
    g.fd = fd;
    g.want_sha = fused || archive_digest != nullptr;
    gz_begin(g);
    enc.begin(g);

    // The pass, slot by slot (S bytes of the tar stream each), as a pipeline over the two staging slots:
    //   host threads   fill slot k+1 (headers, parallel pread at the tar offsets, job list)      | while
    //   copy stream    H2D of slot k (after the hashing kernels that last read this slot's HBM)   | the GPU
    //   ctx stream     SHA-512 kernels over the files of slot k, out of the staged tar stream      | works on
    //   deflate stream DEFLATE + concatenation of slot k, D2H into one of two pinned buffers      | slot k
    //   consumers      file writer and archive digest take that buffer off the producer's thread
    std::atomic<int> first_err{0};
    std::atomic<int64_t> first_err_src{-1};
    struct Filled { int rc = SNAPHASH_OK; std::string err; size_t nj = 0; uint64_t blocks = 0, bytes = 0; double ms = 0; };
    size_t mi = 0; // first member that may still touch the slot being filled (fills run one after another)
    // (runs on a thread of its own; ends by putting the slot's bytes on their way to the GPU, so that the copy of slot
    // k + 1 is behind it when slot k's compression ends and the GPU does not wait for the producer's thread to come round)
    // in_parts (the pass's first slot, on the calling thread): the slot is read, copied and handed to the compressor a
    // piece's worth at a time, so the first chunk kernel starts ~3 ms into the pass instead of after the whole slot's
    // fill and copy (~11 ms); a chunk's output depends on no byte behind its own end (deflate_kernels.hip: matches are
    // cut at the chunk's end, the hash takes three bytes), so what lies beyond a part that has arrived may be anything.
    const uint64_t kPart = (uint64_t)kZPiece * kDeflateChunk;
    auto fill = [&](Slot& sl, uint64_t s0, uint64_t n, Span ev, bool in_parts) { // (its span by value, taken by the calling thread: a fill on a thread of its own never touches the ledger)
        Filled f;
        const double tf0 = now_ms();
        std::vector<ReadOp> ops;
        const int slot_no = (int)(&sl - &c->slot[0]);
        std::vector<MemberHashers::Task> host_tasks; // given out when the slot's bytes are there
        if (!hosted_sizes.empty()) mh.wait_slot(slot_no); // (host threads may still be hashing what this buffer held two slots ago)
        std::vector<TarSegment> segs; // where the regular members' bytes go: the layout itself is tarpack.cpp's
        f.rc = tar_fill_slot(plan, mi, s0, n, sl.h_buf.data(), segs);
        if (f.rc) {
            f.err = "member does not fit a tar header: " + plan.members[mi].name;
            return f;
        }
        for (const TarSegment& sg : segs) {
            if (sg.n) ops.push_back(ReadOp{sg.member, sg.file_off, sg.n, sl.h_buf.data() + sg.slot_off, sg.fin});
            // an empty member is opened and probed all the same (os.Open, io.Copy to EOF): gone, a directory now or no longer
            // empty, it fails the pass like any other; no byte is read, the address (its header's) only keeps the list in order
            else ops.push_back(ReadOp{sg.member, 0, 0, sl.h_buf.data() + (sg.slot_off >= 512 ? sg.slot_off - 512 : 0), true});
            if (fused && hosted_of[sg.member] != 0xffffffffu) {
                host_tasks.push_back(MemberHashers::Task{hosted_of[sg.member], sl.h_buf.data() + (sg.n ? sg.slot_off : 0), sg.n, sg.first, sg.fin, slot_no});
            } else if (fused && stream_of[sg.member] != 0xffffffffu) {
                Job j; // the file's bytes where they lie in the staged tar stream
                j.data = (uint64_t)(uintptr_t)(sl.d_buf.data() + sg.slot_off);
                j.nbytes = sg.n;
                j.total_prev = sg.file_off;
                j.idx = stream_of[sg.member];
                j.flags = (sg.first ? kJobFirst : 0u) | (sg.fin ? kJobFinal : 0u);
                sl.jobs.h[f.nj++] = j;
                f.blocks += padded_blocks(j.nbytes, (j.flags & kJobFinal) != 0);
                f.bytes += j.nbytes;
            }
        }
        if (in_parts) {
            if (hipSetDevice(c->device) != hipSuccess || hipEventRecord(ev.a, c->copy_stream) != hipSuccess) { f.rc = SNAPHASH_EDEVICE; f.err = "H2D failed"; return f; }
            f.rc = gz_slot_begin(g, *enc.parts, n, true, s0 + n >= plan.total);
            if (f.rc) { f.err = c->last_error; return f; }
            size_t o = 0;
            unsigned k = 0;
            std::vector<ReadOp> part;
            for (uint64_t b = 0; b < n; b += kPart, ++k) {
                const uint64_t e = std::min(b + kPart, n);
                part.clear();
                while (o < ops.size() && (uint64_t)(ops[o].dst - sl.h_buf.data()) < e) part.push_back(ops[o++]); // (a member that straddles e is read whole: its rest travels with the next part)
                run_reads(c, srcs, part, first_err, first_err_src);
                if (first_err.load()) break;
                if (c->z_part_ev.size() <= k) c->z_part_ev.resize(k + 1);
                if (c->z_part_ev[k].ensure(hipEventDisableTiming) != hipSuccess) { f.rc = SNAPHASH_EDEVICE; f.err = "hipEventCreate failed"; return f; }
                if (hipMemcpyAsync(sl.d_buf.data() + b, sl.h_buf.data() + b, e - b, hipMemcpyHostToDevice, c->copy_stream) != hipSuccess ||
                    hipEventRecord(c->z_part_ev[k], c->copy_stream) != hipSuccess) { f.rc = SNAPHASH_EDEVICE; f.err = "H2D failed"; return f; }
                f.rc = gz_slot_launch(g, *enc.parts, sl, n, e, c->z_part_ev[k]);
                if (f.rc) { f.err = c->last_error; return f; }
            }
            f.ms = now_ms() - tf0;
            if (hipEventRecord(ev.b, c->copy_stream) != hipSuccess) { f.rc = SNAPHASH_EDEVICE; f.err = "H2D failed"; }
            if (!first_err.load()) mh.give_all(host_tasks);
            return f;
        }
        run_reads(c, srcs, ops, first_err, first_err_src);
        f.ms = now_ms() - tf0;
        if (!first_err.load()) mh.give_all(host_tasks);
        // the slot's HBM was last read by the hashing kernels of two slots ago (its compression has been waited for)
        if (hipSetDevice(c->device) != hipSuccess || (sl.busy && hipStreamWaitEvent(c->copy_stream, sl.done, 0) != hipSuccess) ||
            hipEventRecord(ev.a, c->copy_stream) != hipSuccess ||
            hipMemcpyAsync(sl.d_buf.data(), sl.h_buf.data(), n, hipMemcpyHostToDevice, c->copy_stream) != hipSuccess ||
            hipEventRecord(ev.b, c->copy_stream) != hipSuccess) {
            f.rc = SNAPHASH_EDEVICE;
            f.err = "H2D failed";
        }
        return f;
    };
    std::future<Filled> next;
    try { // no C++ exception (thread creation, allocation) may cross the C boundary
    // (Short first slots -- an eighth, a quarter, half a buffer -- were tried and dropped: what they save at the start
    // they cost in hashing launches, each as long as its longest file whatever the slot holds.)
    Span ev_next;
    if (!rc && plan.total) rc = span_take(c, Ev::H2d, &ev_next);
    const bool first_in_parts = enc.parts && std::min<uint64_t>(S, plan.total) > kPart;
    if (!rc && plan.total && !first_in_parts)
        next = std::async(std::launch::async, fill, std::ref(c->slot[0]), (uint64_t)0, std::min<uint64_t>(S, plan.total), ev_next, false);
    unsigned k = 0;
    for (uint64_t s0 = 0, n = 0; s0 < plan.total && !rc; s0 += n, ++k) {
        n = std::min<uint64_t>(S, plan.total - s0);
        Slot& sl = c->slot[k & 1u];
        const bool parts = k == 0 && first_in_parts;
        const Filled f = parts ? fill(sl, s0, n, ev_next, true) : next.get();
        if (s0 == 0) t_first_fill = now_ms();
        if (f.rc) { rc = fail(c, f.rc, f.err); break; }
        if (first_err.load()) break;
        g.st.fill_ms += f.ms;
        c->stats.blocks += f.blocks;
        c->stats.bytes_hashed += f.bytes;
        if (f.nj) { // SHA-512 of the files, from the same staged bytes; records sl.copied behind the job list's copy
            rc = launch_jobs(c, sl.jobs.h.data(), sl.jobs.d.data(), f.nj, c->hash.d_digests.data(), sl.copied);
            if (rc) break;
            HIP_TRY_BREAK(hipEventRecord(sl.done, c->stream));
            sl.busy = true;
        } else {
            HIP_TRY_BREAK(hipEventRecord(sl.copied, c->copy_stream));
        }
        // The other slot's host buffer is free (its H2D completed before its slot's compression was waited for) and its
        // HBM is only touched again by that fill's own H2D, which waits for the slot's hashing kernels: fill it now.
        if (s0 + n < plan.total) {
            if ((rc = span_take(c, Ev::H2d, &ev_next))) break;
            next = std::async(std::launch::async, fill, std::ref(c->slot[(k + 1) & 1u]), s0 + n, std::min<uint64_t>(S, plan.total - s0 - n), ev_next, false);
        }
        rc = parts ? gz_slot_consume(g, *enc.parts, sl, n, (int)(k & 1u)) : enc.slot(g, sl, n, sl.copied, (int)(k & 1u), s0 == 0, s0 + n >= plan.total);
    }
    } catch (const std::exception& ex) {
        rc = fail(c, SNAPHASH_ENOMEM, std::string("the pipeline could not run: ") + ex.what());
    }
    try {
        if (next.valid()) (void)next.get(); // a fill still in flight after an error
    } catch (const std::exception&) {
    }
    for (Slot& sl : c->slot) sl.busy = false;
    if (!rc && first_err.load()) {
        const int64_t s = first_err_src.load();
        rc = fail(c, SNAPHASH_EIO, (s >= 0 ? plan.members[s].path : std::string("?")) + ": " + strerror(first_err.load()));
    }
    uint8_t arch[64];
    const double t_produced = now_ms();
    if (!rc) {
        const int werr = enc.finish(g, arch);
        if (werr) rc = fail(c, SNAPHASH_EIO, std::string(tarname) + ": " + strerror(werr));
        else if (ftruncate(fd, (off_t)g.out_bytes) != 0 && errno != EINVAL) // (EINVAL: not a regular file -- a pipe, /dev/null -- nothing to cut)
            rc = fail(c, SNAPHASH_EIO, std::string(tarname) + ": " + strerror(errno));
    } else {
        gz_abort(g);
    }
    if (getenv("SNAPHASH_TRACE_TARGZ"))
        fprintf(stderr, "snaphash targz: since entry: walk + tar plan + buffers %.1f ms, output created %.1f, first slot filled %.1f, first piece to the consumers %.1f, "
                "last piece %.1f, producer done %.1f, consumers joined %.1f\n", t_planned - t0, t_opened - t0, t_first_fill - t0, g.t_first_piece - t0, g.t_last_piece - t0, t_produced - t0, now_ms() - t0);
    (void)hipStreamSynchronize(c->copy_stream);
    (void)hipStreamSynchronize(c->z_stream);
    (void)hipStreamSynchronize(c->z2_stream);
    (void)hipStreamSynchronize(c->stream);
    collect_producer_events(c, g, enc);
    c->pending = false;
    std::vector<uint8_t> dig(nstreams * 64 + 64);
    if (!rc && nstreams && hipMemcpy(dig.data(), c->hash.d_digests.data(), nstreams * 64, hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(c, SNAPHASH_EDEVICE, "D2H of the digests failed");
    if (!hosted_sizes.empty()) { // the long members' digests, from their host threads
        if (!rc) mh.wait_all();
        mh.stop();
        if (!rc)
            for (size_t k = 0; k < plan.members.size(); ++k)
                if (hosted_of[k] != 0xffffffffu) memcpy(dig.data() + 64 * (size_t)stream_of[k], mh.digests.data() + 64 * (size_t)hosted_of[k], 64);
    }
    c->stats.streams = nstreams - hosted_sizes.size(); // (the kernels'; the long members count with the host's, below)
    g.st.tar_bytes = plan.total;
    g.st.gz_bytes = g.out_bytes;
    g.st.members = plan.members.size();
    g.st.wall_ms = now_ms() - t0;
    x->targz = g.st;
    if (g.want_sha) { x->ex.host_bytes = g.out_bytes; x->ex.host_streams = 1; }
    x->ex.host_bytes += mh.bytes; // (the long members: MemberHashers)
    x->ex.host_streams += hosted_sizes.size();
    merge_stats(x);
    end_top(x, t_top0_);
    if (rc) { (void)unlink(tarname); return lift(x, c, rc); }
    if (archive_digest && g.want_sha) memcpy(archive_digest, arch, 64);
    if (fused) {
        std::string y;
        rc = emit_yaml(recs, arch, dig.data(), y);
        if (rc) return fail(x, rc, "emit_yaml");
        char* p = (char*)malloc(y.size() + 1);
        if (!p) return fail(x, SNAPHASH_ENOMEM, "malloc");
        memcpy(p, y.data(), y.size());
        p[y.size()] = 0;
        *yaml_out = p;
        if (yaml_len) *yaml_len = y.size();
    }
    return SNAPHASH_OK;
}

int snaphash_tar_create(snaphash_ctx* x, const char* tarname, const char* source_dir, const char* exclude_prefix,
                        char** yaml_out, size_t* yaml_len, uint8_t* archive_digest)
try {
    GzipEncoder enc;
    return tar_create_impl(x, enc, tarname, source_dir, exclude_prefix, nullptr, nullptr, yaml_out, yaml_len, archive_digest);
} catch (...) { // allocation or thread-creation failure: no C++ exception crosses the C boundary
    return SNAPHASH_ENOMEM;
}

int snaphash_tar_create_fn(snaphash_ctx* x, const char* tarname, const char* source_dir, snaphash_keep_fn keep, void* user,
                           char** yaml_out, size_t* yaml_len, uint8_t* archive_digest)
try {
    GzipEncoder enc;
    return tar_create_impl(x, enc, tarname, source_dir, nullptr, keep, user, yaml_out, yaml_len, archive_digest);
} catch (...) { // allocation or thread-creation failure: no C++ exception crosses the C boundary
    return SNAPHASH_ENOMEM;
}

void snaphash_get_targz_stats(const snaphash_ctx* x, snaphash_targz_stats* out)
{
    if (x && out) *out = x->targz;
}

} // extern "C"
