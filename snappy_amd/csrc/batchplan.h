// batchplan.h -- the staging engine's batch policy: how a hashing call is cut into batches, who is served by each and
// where every segment lands in its sub-slot.  Internal.  Pure arithmetic on stream lengths: no HIP call, no engine
// (hash_sources in snaphash_api.cpp is the mechanism that fills, copies and launches what is planned here), so the CPU
// suite drives it over any list of lengths (tests/batchplan_host_harness.cpp).  DESIGN.md sec. 5.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "sha512_kernels.h"

namespace snaphash {

constexpr uint64_t kAlign = 256;          // placement of a segment inside a staging buffer
constexpr uint64_t kMinSegment = 32u << 10;    // least a FILE stream is given of a slot, unless it ends there (a pread per segment; an open + close
                                               // too once the call holds more descriptors than its budget, FdCache)
constexpr uint64_t kMinSegmentMem = 16u << 10; // the same for a stream in caller memory (a copy has no such cost)
constexpr uint32_t kTargetStreams = 4096; // streams per batch the engine aims for (keeps the kernel ahead of PCIe)
constexpr uint64_t kHold = 16u << 10;    // what the batch that would be the last leaves of every stream for one more (BatchPlanner::next)

struct Source {
    const char* path = nullptr;   // file source
    const uint8_t* mem = nullptr; // memory source
    uint64_t len = 0;
    uint64_t gpu_len = 0;         // bytes this engine hashes: == len (whole stream, digest out) or a multiple of
                                  // 128 below len (prefix only: the chaining value is handed to a host thread)
};

struct ReadOp { uint32_t src; uint64_t off; uint64_t n; uint8_t* dst; bool to_eof; };

// lab knobs, read once a CALL (so that one process can alternate settings between passes: tools/ramp_ab.py)
struct BatchKnobs {
    size_t new_cap = 1024;   // streams a batch may BEGIN (file sources, trees of more than 2 048 streams); SNAPHASH_NEW_PER_BATCH=0: no cap
    bool hold_back = true;   // the last batch of a link-bound job is cut in two; SNAPHASH_HOLD_BACK=0: not
    unsigned ramp_shift = 3; // the first batch of a large job is S_full >> this; SNAPHASH_RAMP_SHIFT, 1..8
    // ... of a job of many streams (link-bound), "first fraction in 1/64ths, growth per batch in percent": 24,115 = three
    // eighths of a batch first, 15 % more each time (BatchPlanner::next); SNAPHASH_RAMP_MANY=a,b with 1 <= a <= 64, 100 <= b <= 400
    unsigned ramp_first64 = 24, ramp_growth_pct = 115;
    static BatchKnobs from_env();
};

// Slots and sub-slots of a call.  slot_caps: what the engine's three staging buffers hold already (0 = not there).
struct BatchGeometry {
    unsigned nslots;     // staging buffers the call uses: a third one when it has more than two buffers' worth of bytes
    uint64_t slot_bytes; // bytes of each
    uint64_t S_full;     // bytes of a sub-slot, the largest batch
    unsigned per_slot, nsub; // sub-slots in a buffer, and in all
};
BatchGeometry batch_geometry(uint64_t job_bytes, size_t n, uint64_t staging, const uint64_t slot_caps[3], bool from_memory);

struct Batch {
    uint64_t S = 0;      // bytes this batch was planned into (<= S_full)
    uint64_t used = 0;   // bytes of the sub-slot it takes: what the H2D copy moves
    size_t nj = 0;       // segments (jobs written)
    size_t n_new = 0;    // streams it begins, where that is capped (BatchKnobs::new_cap; 0 otherwise)
    uint64_t blocks = 0; // SHA-512 compression-function calls of its segments (padding included)
};

// The batches of one call, one next() each while active is not empty.  src must outlive the planner.
struct BatchPlanner {
    BatchPlanner(const Source* src, size_t n, uint64_t job_bytes, uint64_t S_full, const BatchKnobs& knobs);
    // Plans the next batch into jobs[0 .. active.size()) and ops (cleared first; a segment of 0 bytes has no read).  A
    // segment at offset `at` of the sub-slot gets the device address d_base + at and is read to h_base + at.
    Batch next(Job* jobs, std::vector<ReadOp>& ops, uint64_t h_base, uint64_t d_base);

    const Source* src;
    size_t n;
    uint64_t job_bytes, S_full;
    BatchKnobs knobs;
    bool from_memory;
    uint64_t seg_floor;
    size_t n_active0;
    std::vector<uint64_t> done;   // per stream: bytes planned so far
    std::vector<uint32_t> active; // streams not finished, in the order the next batch looks at them
    std::vector<uint32_t> still, skipped, floor_still; // next()'s scratch: who is served next time
    bool held_back = false; // the last batch of a link-bound job has been cut in two
    unsigned batch = 0;     // batches planned so far
};

// A 64-bit mix over a batch's segments in the order planned: idx, offset in the sub-slot, nbytes, total_prev, flags.
uint64_t batch_checksum(const Job* jobs, size_t nj, uint64_t d_base);
// The line of SNAPHASH_TRACE_BATCHES (jobs as next() left them, before launch_jobs sorts them; left = active.size() afterwards).
void trace_batch(FILE* f, int engine, unsigned batch, const Batch& b, const Job* jobs, uint64_t d_base, size_t left);

} // namespace snaphash
