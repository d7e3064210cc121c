// The staging engine's batch policy (snappy_amd/csrc/batchplan.cpp) on the CPU: plans one call the way hash_sources does,
// against made-up slot addresses that nothing dereferences, checks every segment of every batch, and prints the batches in
// the engine's own trace format (SNAPHASH_TRACE_BATCHES) for tests/test_batchplan_host.py to compare.
//
//   batchplan_host plan SPEC    SPEC is a text file:  staging from_memory cap0 cap1 cap2
//                                                     new_cap hold_back ramp_shift ramp_first64 ramp_growth_pct
//                                                     n, then n lines "len gpu_len"
//   batchplan_host segments SPEC  the same, and a line "seg BATCH STREAM TOTAL_PREV NBYTES FLAGS" for every segment
//   batchplan_host knobs        prints BatchKnobs::from_env()
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../snappy_amd/csrc/batchplan.cpp"

using namespace snaphash;

#define CHECK(cond, ...)                                                       \
    do {                                                                       \
        if (!(cond)) {                                                         \
            printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond);             \
            printf(__VA_ARGS__);                                               \
            printf("\n");                                                      \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

static int plan(const char* spec, bool segments)
{
    FILE* f = fopen(spec, "r");
    CHECK(f, "cannot open %s", spec);
    uint64_t staging = 0, caps[3] = {0, 0, 0};
    int from_memory = 0, hold = 1;
    BatchKnobs knobs;
    size_t n = 0;
    CHECK(fscanf(f, "%" SCNu64 " %d %" SCNu64 " %" SCNu64 " %" SCNu64, &staging, &from_memory, &caps[0], &caps[1], &caps[2]) == 5, "header");
    CHECK(fscanf(f, "%zu %d %u %u %u", &knobs.new_cap, &hold, &knobs.ramp_shift, &knobs.ramp_first64, &knobs.ramp_growth_pct) == 5, "knobs");
    knobs.hold_back = hold != 0;
    CHECK(fscanf(f, "%zu", &n) == 1 && n > 0, "n");
    std::vector<Source> src(n);
    static const uint8_t some_byte = 0;
    uint64_t job_bytes = 0;
    for (size_t i = 0; i < n; ++i) {
        CHECK(fscanf(f, "%" SCNu64 " %" SCNu64, &src[i].len, &src[i].gpu_len) == 2, "stream %zu", i);
        CHECK(src[i].gpu_len == src[i].len || (src[i].gpu_len < src[i].len && src[i].gpu_len % 128 == 0), "stream %zu: a prefix is whole blocks", i);
        if (from_memory) src[i].mem = &some_byte; else src[i].path = "/nonexistent";
        job_bytes += src[i].gpu_len;
    }
    fclose(f);

    const BatchGeometry g = batch_geometry(job_bytes, n, staging, caps, from_memory != 0);
    printf("geometry: nslots %u, slot_bytes %" PRIu64 ", S_full %" PRIu64 ", per_slot %u, nsub %u\n", g.nslots, g.slot_bytes, g.S_full, g.per_slot, g.nsub);
    CHECK(g.nslots == 2 || g.nslots == 3, "nslots");
    CHECK(g.slot_bytes <= staging && g.S_full <= g.slot_bytes && g.per_slot >= 1 && (uint64_t)g.per_slot * g.S_full <= g.slot_bytes && g.nsub == g.nslots * g.per_slot, "geometry");
    for (unsigned k = 0; k < g.nslots; ++k) CHECK(g.slot_bytes >= (caps[k] < staging ? caps[k] : staging), "a slot that is there is used whole");

    BatchPlanner p(src.data(), n, job_bytes, g.S_full, knobs);
    std::vector<Job> jobs(n ? n : 1);
    std::vector<ReadOp> ops;
    std::vector<uint64_t> seen(n, 0);
    std::vector<uint32_t> nseg(n, 0), in_batch(n, 0);
    const bool capped = knobs.new_cap != 0 && !from_memory && p.n_active0 > 2048;
    unsigned hold_backs = 0;
    size_t max_begun = 0;
    while (!p.active.empty()) {
        const unsigned q = p.batch % g.nsub;
        // addresses as the engine lays its sub-slots out, 4 GiB apart per buffer; never dereferenced
        const uint64_t h_base = 0x100000000000ull + ((uint64_t)(q / g.per_slot) << 32) + (uint64_t)(q % g.per_slot) * g.S_full;
        const uint64_t d_base = 0x700000000000ull + ((uint64_t)(q / g.per_slot) << 32) + (uint64_t)(q % g.per_slot) * g.S_full;
        const unsigned batch = p.batch;
        const size_t before = p.active.size();
        const bool held_before = p.held_back;
        CHECK(before <= jobs.size(), "more active streams than streams");
        const Batch b = p.next(jobs.data(), ops, h_base, d_base);
        CHECK(p.batch == batch + 1 && batch < 1000000, "the planner terminates");
        CHECK(b.nj <= before, "batch %u: more segments than active streams", batch);
        CHECK(b.S <= g.S_full && b.used <= b.S, "batch %u: used %" PRIu64 " S %" PRIu64, batch, b.used, b.S);
        CHECK(b.nj > 0 || p.active.size() < before || p.held_back != held_before, "batch %u: serves nobody", batch);
        // A batch that holds back is told by what it plans, not by the planner's word: nobody ends in it, every stream it
        // serves stops kHold (and what alignment rounds off) short of its end ...
        bool holds_back = b.nj > 0;
        uint64_t end = 0, blocks = 0;
        size_t begun = 0, op = 0;
        for (size_t k = 0; k < b.nj; ++k) {
            const Job& j = jobs[k];
            CHECK(j.idx < n, "batch %u segment %zu: idx", batch, k);
            const Source& s = src[j.idx];
            const uint64_t at = j.data - d_base;
            CHECK(j.data >= d_base && at % kAlign == 0 && at >= end && at + j.nbytes <= b.S, "batch %u segment %zu: at %" PRIu64 " + %" PRIu64 " after %" PRIu64, batch, k, at, j.nbytes, end);
            end = at + j.nbytes;
            CHECK(in_batch[j.idx] != batch + 1, "batch %u: stream %u twice", batch, j.idx);
            in_batch[j.idx] = batch + 1;
            CHECK(j.total_prev == seen[j.idx], "batch %u stream %u: total_prev %" PRIu64 ", hashed before %" PRIu64, batch, j.idx, j.total_prev, seen[j.idx]);
            CHECK(((j.flags & kJobFirst) != 0) == (nseg[j.idx] == 0) && (j.flags & ~(kJobFirst | kJobFinal)) == 0, "batch %u stream %u: first flag", batch, j.idx);
            begun += nseg[j.idx] == 0 && s.gpu_len != 0;
            ++nseg[j.idx];
            seen[j.idx] += j.nbytes;
            CHECK(seen[j.idx] <= s.gpu_len, "batch %u stream %u: past its end", batch, j.idx);
            const bool last = seen[j.idx] == s.gpu_len, fin = (j.flags & kJobFinal) != 0;
            CHECK(fin == (last && s.gpu_len == s.len), "batch %u stream %u: final flag", batch, j.idx);
            const uint64_t rem_after = s.gpu_len - seen[j.idx];
            holds_back = holds_back && rem_after >= kHold && rem_after < kHold + kAlign;
            if (!last) CHECK(j.nbytes > 0 && j.nbytes % 128 == 0, "batch %u stream %u: a segment that is not the last is whole blocks (%" PRIu64 ")", batch, j.idx, j.nbytes);
            if (j.nbytes == 0) CHECK(s.gpu_len == 0 && s.len == 0, "batch %u stream %u: an empty segment of a non-empty stream", batch, j.idx);
            blocks += padded_blocks(j.nbytes, fin);
            if (segments) printf("seg %u %u %" PRIu64 " %" PRIu64 " %u\n", batch, j.idx, j.total_prev, j.nbytes, j.flags);
            if (j.nbytes) { // its read (the PLANNER's reads: the engine adds an open-and-probe of its own for an empty file, hash_sources)
                CHECK(op < ops.size(), "batch %u: a segment without a read", batch);
                const ReadOp& r = ops[op++];
                CHECK(r.src == j.idx && r.off == j.total_prev && r.n == j.nbytes && (uint64_t)(uintptr_t)r.dst == h_base + at, "batch %u stream %u: read", batch, j.idx);
                CHECK(r.to_eof == (fin && !from_memory), "batch %u stream %u: to_eof", batch, j.idx);
            }
        }
        CHECK(op == ops.size(), "batch %u: %zu reads for %zu segments with bytes", batch, ops.size(), op);
        CHECK(end == b.used && blocks == b.blocks, "batch %u: used / blocks", batch);
        if (capped) CHECK(begun <= b.n_new && b.n_new <= knobs.new_cap, "batch %u begins %zu streams (n_new %zu)", batch, begun, b.n_new);
        if (begun > max_begun) max_begun = begun;
        // (... and it passes over nobody who has more than a batch-behind's worth left: 5 000 x 256 KiB served 16 KiB at a time
        // leave 16 KiB of 4 096 streams too, in a batch that had no room for the other 904)
        for (size_t k = 0; holds_back && k < p.active.size(); ++k) {
            const uint32_t id = p.active[k];
            if (in_batch[id] != batch + 1 && src[id].gpu_len - seen[id] > kHold + kHold / 2) holds_back = false;
        }
        CHECK(holds_back == (p.held_back && !held_before), "batch %u: holds back %d, the planner says %d", batch, (int)holds_back, (int)(p.held_back && !held_before));
        hold_backs += holds_back;
        trace_batch(stdout, 0, batch, b, jobs.data(), d_base, p.active.size());
    }
    for (size_t i = 0; i < n; ++i) {
        CHECK(seen[i] == src[i].gpu_len, "stream %zu: %" PRIu64 " of %" PRIu64 " bytes planned", i, seen[i], src[i].gpu_len);
        if (src[i].len == 0) CHECK(nseg[i] == 1, "empty stream %zu: %u segments", i, nseg[i]);
        else if (src[i].gpu_len == 0) CHECK(nseg[i] == 0, "stream %zu, prefix of 0 bytes: %u segments", i, nseg[i]);
        else CHECK(nseg[i] >= 1, "stream %zu", i);
    }
    if (job_bytes + kAlign * n <= g.S_full) CHECK(p.batch == 1, "a job that fits one slot is one batch, not %u", p.batch);
    CHECK(hold_backs <= 1 && (knobs.hold_back || hold_backs == 0), "hold-backs %u", hold_backs);
    printf("summary: %u batches, %u hold-backs, most streams begun by a batch %zu\n", p.batch, hold_backs, max_begun);
    printf("plan ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 3 && !strcmp(argv[1], "plan")) return plan(argv[2], false);
    if (argc == 3 && !strcmp(argv[1], "segments")) return plan(argv[2], true);
    if (argc == 2 && !strcmp(argv[1], "knobs")) {
        const BatchKnobs k = BatchKnobs::from_env();
        printf("new_cap %zu hold_back %d ramp_shift %u ramp_first64 %u ramp_growth_pct %u\nknobs ok\n", k.new_cap, (int)k.hold_back, k.ramp_shift, k.ramp_first64, k.ramp_growth_pct);
        return 0;
    }
    fprintf(stderr, "usage: %s plan SPEC | segments SPEC | knobs\n", argv[0]);
    return 2;
}
