// batchplan.cpp -- see batchplan.h.  Host-only (no HIP call): the CPU suite drives it through tests/batchplan_host_harness.cpp.
#include "batchplan.h"

#include <stdlib.h>

#include <algorithm>

#include "sha512_core.h"

namespace snaphash {

BatchKnobs BatchKnobs::from_env()
{
    BatchKnobs k;
    if (const char* e = getenv("SNAPHASH_NEW_PER_BATCH")) k.new_cap = (size_t)strtoul(e, nullptr, 10);
    if (const char* e = getenv("SNAPHASH_HOLD_BACK")) k.hold_back = atoi(e) != 0;
    if (const char* e = getenv("SNAPHASH_RAMP_SHIFT")) k.ramp_shift = (unsigned)std::min<unsigned long>(std::max<unsigned long>(strtoul(e, nullptr, 10), 1), 8);
    if (const char* e = getenv("SNAPHASH_RAMP_MANY")) {
        unsigned a = 0, b = 0;
        if (sscanf(e, "%u,%u", &a, &b) == 2 && a >= 1 && a <= 64 && b >= 100 && b <= 400) { k.ramp_first64 = a; k.ramp_growth_pct = b; }
    }
    return k;
}

BatchGeometry batch_geometry(uint64_t job_bytes, size_t n, uint64_t staging, const uint64_t slot_caps[3], bool from_memory)
{
    BatchGeometry g;
    g.nslots = job_bytes > 2 * staging ? 3u : 2u;
    // slots as large as the job needs, in powers of two from 8 MiB up to the engine's staging size (they grow when a
    // larger job comes by, and never shrink)
    uint64_t slot_bytes = std::min<uint64_t>(staging, 8u << 20);
    while (slot_bytes < staging && slot_bytes < job_bytes / 2 + kAlign * n) slot_bytes <<= 1;
    slot_bytes = std::min(slot_bytes, staging);
    for (unsigned k = 0; k < g.nslots; ++k) slot_bytes = std::max(slot_bytes, std::min(slot_caps[k], staging)); // what is there already is used
    g.slot_bytes = slot_bytes;
    const uint64_t seg_floor = from_memory ? kMinSegmentMem : kMinSegment;
    // The batch: a job of more than a buffer is cut into about two dozen batches (32 MiB at least, a buffer at most, and
    // room for every stream's floor), each in a sub-slot of the buffers; so many are in flight that the fill runs
    // ahead of the copy engine and the copy engine ahead of the kernels.
    uint64_t S_full = slot_bytes;
    if (job_bytes + kAlign * n > slot_bytes && (slot_bytes & (slot_bytes - 1)) == 0 && slot_bytes > (32u << 20)) {
        S_full = 32u << 20;
        while (S_full < slot_bytes && (S_full < job_bytes / 24 || S_full < (seg_floor + kAlign) * std::min<uint64_t>(n, kTargetStreams))) S_full <<= 1;
    }
    g.S_full = S_full;
    g.per_slot = (unsigned)(slot_bytes / S_full);
    g.nsub = g.nslots * g.per_slot;
    return g;
}

BatchPlanner::BatchPlanner(const Source* src, size_t n, uint64_t job_bytes, uint64_t S_full, const BatchKnobs& knobs)
    : src(src), n(n), job_bytes(job_bytes), S_full(S_full), knobs(knobs), from_memory(n != 0 && src[0].mem != nullptr),
      seg_floor(from_memory ? kMinSegmentMem : kMinSegment), done(n, 0)
{
    active.reserve(n);
    for (size_t i = 0; i < n; ++i)
        if (src[i].gpu_len > 0 || src[i].len == 0) active.push_back((uint32_t)i); // a prefix of 0 bytes needs no launch
    // longest first: the streams that set the makespan are served in every batch from the first one on
    std::stable_sort(active.begin(), active.end(), [&](uint32_t a, uint32_t b) { return src[a].gpu_len > src[b].gpu_len; });
    n_active0 = active.size();
    still.reserve(n_active0);
}

Batch BatchPlanner::next(Job* jobs, std::vector<ReadOp>& ops, uint64_t h_base, uint64_t d_base)
{
    const size_t new_cap = knobs.new_cap;
    const unsigned ramp_shift = knobs.ramp_shift, ramp_first64 = knobs.ramp_first64, ramp_growth_pct = knobs.ramp_growth_pct;
    // What a stream gets of this slot: its share by remaining length (so that long and short streams end in the
    // same batch -- a long stream served a fixed slice per batch would still be running, alone, long after the
    // others: the per-stream rate of the kernels is what it is), but at least a floor (a file is opened once per
    // batch it appears in).  Equal streams (config 2) fill a slot kTargetStreams at a time, as before.
    // Both ends of a job of several slots are tapered: nothing overlaps the first fill and the
    // first copy, and nothing overlaps the last copy and the last kernel, so the first batches are 1/8, 1/4, 1/2 of
    // a slot and the last ones halve what is left -- invisible on a 10 GiB job, a fifth of the time of the 1.3 GiB
    // shard one of eight ranks gets.  A job that fits one slot is one batch.
    long double total_rem = 0;
    size_t n_started = 0;
    for (uint32_t id : active) { total_rem += (long double)(src[id].gpu_len - done[id]); n_started += done[id] != 0; }
    uint64_t S = S_full;
    if (job_bytes + kAlign * n > S_full) {
        if (n_active0 > 2048 && ramp_growth_pct > 100) {
            // Many streams: the link is the bound, and the fill threads are only ~1.3 x as fast as the link (75 against
            // 57 GB/s).  The link idles while the first batch is filled, and again before every batch that takes longer
            // to fill than its predecessor takes to copy -- doubling batches (rounds 1-4: 1/8, 1/4, 1/2, 1) lose
            // S x (2 / 75 - 1 / 57 GB/s) at every step: 3.5 ms in all on config 2, measured 3.6
            // (profiles/r05_tree_events_before.txt).  A batch that grows by less than fill rate / link rate a step never
            // makes the link wait: three eighths of a batch first, 15 % more each time (tools/ramp_ab.py; profiles/r05_ramp.txt:
            // the link idle 1.4 + 1.1 ms at the start instead of 1.0 + 4.8).
            double f = (double)ramp_first64 / 64.0;
            for (unsigned k = 0; k < batch && f < 1.0; ++k) f *= (double)ramp_growth_pct / 100.0;
            if (f < 1.0) S = std::max<uint64_t>((uint64_t)((double)S_full * f) & ~(uint64_t)(kAlign - 1), std::min<uint64_t>(S_full, 1u << 20));
        } else if (batch < ramp_shift) {
            // ... but never so small that only some streams get their floor: a batch costs the kernel chain its LARGEST
            // share's time, so 256 streams at 32 KiB cost what all 1 250 at 32 KiB would (the file-source shard's first
            // three batches: 0.75 ms of kernel each for 8, 16 and 32 MiB; profiles/r04_shard_trace.txt)
            // (That is a concern of jobs bound by their kernel chain: up to ~2 000 streams, whose 44 MB/s each do not
            // outrun the link.  With more streams the link is the bound and the first copy should start early: the C2
            // tree's first batch was a whole 256 MiB buffer, 4 ms of fill with the link idle.)
            // (Finer steps -- x 1.4 a batch from 16 MiB, eight of them -- were tried for that regime and left the link idle
            // MORE, 4.5 ms against 3.5: every batch costs ~0.4 ms of planning and hand-over whatever its size.)
            const uint64_t every = active.size() <= 2048 ? std::min<uint64_t>(S_full, (seg_floor + kAlign) * (uint64_t)active.size()) : 0;
            S = std::max<uint64_t>({(S_full >> (ramp_shift - batch)) & ~(uint64_t)(kAlign - 1), every & ~(uint64_t)(kAlign - 1), std::min<uint64_t>(S_full, 1u << 20)});
        }
        if (total_rem < 2 * (long double)S) { // the end: half of what is left, while every stream can still get its floor
            const uint64_t half = ((uint64_t)(total_rem / 2) + kAlign * active.size()) & ~(uint64_t)(kAlign - 1);
            const uint64_t least = std::max<uint64_t>(S_full >> 5, (seg_floor + kAlign) * active.size());
            if (half >= least) S = std::min(S, half);
        }
    }
    // A file's FIRST segment costs an open(), and every open of a process takes the lock of its one descriptor table
    // (~3 us alone, ~19 us each with twelve threads at it).  A tree of many files used to begin all of
    // them within its first four batches -- config 2: 10 001 opens in the first 480 MiB, whose fills ran at 40-50 GB/s
    // where later ones run at 76, and the link idled 6 ms of the ramp (profiles/r05_tree_events_before.txt).  So a
    // batch begins at most new_cap streams; the rest of it goes to streams already open (kept descriptors: a pread
    // each).  Streams nobody has begun go in front of those served at the floor, so every batch begins its share.
    const bool cap_new = new_cap != 0 && !from_memory && n_active0 > 2048;
    const size_t n_serve = cap_new ? std::min<size_t>(kTargetStreams, n_started + std::min<size_t>(new_cap, active.size() - n_started)) : kTargetStreams;
    const uint64_t floor_q = std::max<uint64_t>(seg_floor, (S / std::max<size_t>(1, n_serve)) & ~(uint64_t)(kAlign - 1));
    // What the shares are taken of: the batch less the alignment every segment may cost.  Without that the shares of
    // ALL streams came to a whole batch, the padding pushed the last dozen streams of the list out of every batch, and
    // they were hashed at the end, alone, at 44 MB/s each (5 000 x 1 MiB: the last four kernels took 26 ms instead of
    // 6, 114 ms for a job whose copies take 92; profiles/r04_shard_trace.txt).
    const uint64_t pad = kAlign * (uint64_t)active.size();
    const uint64_t S_share = pad < S / 2 ? S - pad : S;

    ops.clear();
    Batch b;
    b.S = S;
    size_t nj = 0;
    uint64_t used = 0;
    // Who is served next time.  A batch cannot always serve every stream (more streams than it has floors for: 5 000 x
    // 1 MiB at a floor of 64 KiB, 100 000 small files); round 3 then served the SAME leading streams batch after batch and
    // the ones behind them only when those were done -- 904 of 5 000 streams hashed at the end, alone, 290 KiB a batch
    // at 44 MB/s: kernels of 6-9 ms behind copies of 4.7 (profiles/r04_shard_trace.txt).  Now the streams a batch had
    // no room for go FIRST in the next one, in front of those that were served at the floor; streams whose share by
    // length exceeds the floor (the long ones that set the makespan) stay in front of both and are served every time.
    still.clear();
    skipped.clear();
    floor_still.clear();
    // The last batch of a link-bound job: nothing overlaps its kernel, which takes what its LARGEST share takes at a
    // stream's 44 MB/s -- 64 KiB shares: 1.5-1.7 ms behind the last copy (profiles/r05_tree_events_before.txt).  So the batch
    // that would be the last leaves 16 KiB (kHold) of every stream behind for one more, whose kernel is 0.4 ms.
    // (... of streams that HAVE that much left -- more than the 24 KiB below which a stream goes to the batch behind whole, on
    // average: 5 000 x 8 KiB made the batch in front of the last an EMPTY one, profiles/r05_small_files.txt.  Config 2's last
    // batch has 26 KiB a stream: a first version of this test asked for 32 and switched the hold-back off for it, +1.5 ms.)
    const bool hold_back = knobs.hold_back && !held_back && n_active0 > 2048 && total_rem <= (long double)S_share && total_rem > (long double)(8u << 20) &&
                           total_rem > (long double)(kHold + kHold / 2) * (long double)active.size();
    if (hold_back) held_back = true;
    bool full = false;
    size_t n_new = 0;
    // (one division a batch, not one a stream: the engine's thread plans 4 096 segments a batch between two fills, and in
    // the ramp nothing hides that)
    const bool share_all = total_rem > (long double)S;
    const long double share_ratio = share_all ? (long double)S_share / total_rem : 1.0L;
    for (size_t ai = 0; ai < active.size(); ++ai) {
        const uint32_t id = active[ai];
        if (full) { skipped.insert(skipped.end(), active.begin() + (ptrdiff_t)ai, active.end()); break; } // nobody behind a full batch is looked at
        if (cap_new && done[id] == 0 && src[id].gpu_len != 0) {
            if (n_new >= new_cap) { skipped.push_back(id); continue; } // begun by a later batch
            ++n_new;
        }
        const uint64_t rem = src[id].gpu_len - done[id];
        uint64_t quota = share_all ? (uint64_t)((long double)rem * share_ratio) : rem;
        const bool at_floor = (quota & ~(uint64_t)(kAlign - 1)) < floor_q;
        quota = std::max(quota & ~(uint64_t)(kAlign - 1), floor_q); // a multiple of 128: segments are whole blocks
        uint64_t take = rem <= quota ? rem : quota;
        if (hold_back) {
            if (rem <= kHold + kHold / 2) { skipped.push_back(id); continue; } // all of it in the batch behind this one
            take = std::min<uint64_t>(take, (rem - kHold) & ~(uint64_t)(kAlign - 1));
        }
        const uint64_t at = (used + kAlign - 1) & ~(uint64_t)(kAlign - 1);
        if (at + take > S) { full = true; skipped.push_back(id); continue; }
        const bool last = take == rem;
        const bool fin = last && src[id].gpu_len == src[id].len;
        Job j;
        j.data = d_base + at;
        j.nbytes = take;
        j.total_prev = done[id];
        j.idx = id;
        j.flags = (done[id] == 0 ? kJobFirst : 0u) | (fin ? kJobFinal : 0u);
        jobs[nj++] = j;
        if (take) ops.push_back(ReadOp{id, done[id], take, (uint8_t*)(uintptr_t)(h_base + at), fin && src[id].path != nullptr});
        used = at + take;
        done[id] += take;
        b.blocks += padded_blocks(take, fin);
        if (!last) (at_floor ? floor_still : still).push_back(id);
    }
    still.insert(still.end(), skipped.begin(), skipped.end());
    still.insert(still.end(), floor_still.begin(), floor_still.end());
    active.swap(still);
    ++batch;
    b.used = used;
    b.nj = nj;
    b.n_new = n_new;
    return b;
}

uint64_t batch_checksum(const Job* jobs, size_t nj, uint64_t d_base)
{
    uint64_t h = 0x9e3779b97f4a7c15ull;
    auto mix = [&h](uint64_t v) { h = (h ^ v) * 0xff51afd7ed558ccdull; h ^= h >> 32; };
    for (size_t k = 0; k < nj; ++k) {
        mix(jobs[k].idx);
        mix(jobs[k].data - d_base);
        mix(jobs[k].nbytes);
        mix(jobs[k].total_prev);
        mix(jobs[k].flags);
    }
    return h;
}

void trace_batch(FILE* f, int engine, unsigned batch, const Batch& b, const Job* jobs, uint64_t d_base, size_t left)
{
    uint64_t mx = 0;
    for (size_t k = 0; k < b.nj; ++k) mx = std::max<uint64_t>(mx, jobs[k].nbytes);
    fprintf(f, "snaphash engine %d: batch %u: S %llu, %zu segments, %llu bytes, largest share %llu, %zu streams left behind, checksum %016llx\n", engine, batch,
            (unsigned long long)b.S, b.nj, (unsigned long long)b.used, (unsigned long long)mx, left, (unsigned long long)batch_checksum(jobs, b.nj, d_base));
}

} // namespace snaphash
