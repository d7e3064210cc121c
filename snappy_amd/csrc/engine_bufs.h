// engine_bufs.h -- an engine's scratch (DevCtx, snaphash_api.cpp), grouped by the code that uses it.  Internal.
//
// A group's ensure() sizes every buffer of the group for a job, or on any failure leaves every one of them empty; each()
// lists the group's buffers once, for the engine's release and its footprint (snaphash_get_engine_info).  Pinned
// buffers take the engine's NUMA node, or -1 where the runtime places them (hipHostMallocDefault).
#pragma once
#include <algorithm>

#include "bcj_kernels.h"
#include "bz2_check_kernels.h"
#include "bzip2_host.h"
#include "bzip2_enc_kernels.h"
#include "bzip2_kernels.h"
#include "crc_kernels.h"
#include "deflate_check_kernels.h"
#include "deflate_kernels.h"
#include "devbuf.h"
#include "gpu_handles.h"
#include "inflate_core.h"
#include "inflate_kernels.h"
#include "lzma2_check_kernels.h"
#include "sha256_kernels.h"
#include "sha512_kernels.h"
#include "xz_host.h"
#include "xz_enc_kernels.h"
#include "xz_kernels.h"

namespace snaphash {

// a table built in pinned memory and its HBM twin, n entries each
template <class T> struct Twin {
    HostBuf<T> h;
    DevBuf<T> d;
    size_t size() const { return d.size(); }
    hipError_t ensure(size_t n)
    {
        hipError_t e = h.reserve(n, -1);
        if (!e) e = d.reserve(n);
        if (e) each(Release());
        return e;
    }
    template <class F> void each(F&& f) { f(h); f(d); }
};

// job arrays hold 1024 jobs at least
struct JobBufs : Twin<Job> {
    hipError_t ensure(size_t n) { return Twin::ensure(std::max<size_t>(n, 1024)); }
};

// A staging buffer (pinned, and its HBM twin with 256 bytes of slack: the deflate kernel peeks 3 bytes past a chunk) and
// the job array of the batch staged in it.
struct Slot {
    HostBuf<uint8_t> h_buf;
    DevBuf<uint8_t> d_buf;
    JobBufs jobs;
    Event done;   // kernel of the batch staged in this slot has finished
    Event copied; // H2D of this slot's data + jobs has finished
    bool busy = false;
    uint64_t cap() const { return h_buf.size(); } // bytes both hold (the engine's staging size, or less while only small jobs have come by)
    hipError_t ensure(uint64_t bytes, int node)
    {
        hipError_t e = h_buf.reserve(bytes, node);
        if (!e) e = d_buf.reserve(bytes + 256);
        if (e) { h_buf.reset(); d_buf.reset(); }
        return e;
    }
    template <class F> void each(F&& f) { f(h_buf); f(d_buf); jobs.each(f); }
};

// A batch of the hashing engine lives in a sub-slot: a piece of one of the engine's staging buffers with its own job
// array and events.  A job of several buffers' worth is cut into batches much smaller than a buffer (hash_sources):
// when the streams' own rate is about the link's (a rank's shard of config 4: 1 250 streams x 44 MB/s = 55 GB/s), fill,
// copy and kernel are three stages of equal length and only many small batches in flight keep all three busy.
struct SubSlot {
    JobBufs jobs;
    Event done;   // kernel of the batch staged here has finished
    Event copied; // H2D of this batch's jobs has finished
    bool busy = false;
};

// hashing: the chaining values and digests of a call's streams (64 bytes each), the device-resident entry point's jobs
struct HashBufs {
    JobBufs jobs;
    DevBuf<uint64_t> d_state;
    DevBuf<uint8_t> d_digests;
    // njobs = 0: the job array as it is
    hipError_t ensure(size_t streams, bool with_digests, size_t njobs = 0)
    {
        hipError_t e = d_state.reserve(streams * 8);
        if (!e && with_digests) e = d_digests.reserve(streams * 64);
        if (!e && njobs) e = jobs.ensure(njobs);
        if (e) each(Release());
        return e;
    }
    template <class F> void each(F&& f) { jobs.each(f); f(d_state); f(d_digests); }
};

// block-parallel DEFLATE (row f3, targz.inc), per chunk of a staging slot: output slots, the parse, sizes, offsets,
// the compacted piece, and its way back to the host
struct DeflateBufs {
    DevBuf<uint8_t> d_slots, d_out;
    DevBuf<uint32_t> d_toks; // the deflate kernel's parse, kDeflateTokWords a chunk
    DevBuf<uint32_t> d_sizes;
    DevBuf<uint64_t> d_prefix;
    HostBuf<uint32_t> h_sizes;
    HostBuf<uint64_t> h_prefix;
    HostBuf<uint8_t> h_out[2]; // double-buffered: the consumers read one while the next D2H fills the other
    Twin<DfCheckVerdict> chk;  // the self-check's verdicts, a chunk each: sized by the call that asks for the check (targz.inc), empty otherwise
    size_t chunks() const { return d_sizes.size(); }
    hipError_t ensure(size_t nch, int node)
    {
        hipError_t e = d_slots.reserve(nch * kDeflateSlot);
        if (!e) e = d_out.reserve(nch * kDeflateSlot);
        if (!e) e = d_toks.reserve(nch * kDeflateTokWords);
        if (!e) e = d_sizes.reserve(nch);
        if (!e) e = d_prefix.reserve(nch);
        if (!e) e = h_sizes.reserve(nch, node);
        if (!e) e = h_prefix.reserve(nch, node);
        for (HostBuf<uint8_t>& b : h_out)
            if (!e) e = b.reserve(nch * kDeflateSlot, node);
        if (e) each(Release());
        return e;
    }
    template <class F> void each(F&& f) { f(d_slots); f(d_out); f(d_toks); f(d_sizes); f(d_prefix); f(h_sizes); f(h_prefix); f(h_out[0]); f(h_out[1]); chk.each(f); }
};

// GPU inflate (row f5, unpack.inc): the compressed piece (+16 bytes the bit reader may read past it) and its candidates,
// the speculative segments' slots and results, the linked chain, the hole counters, the window in front of the piece,
// and the decoded bytes (grown by DecodedStream, unpack.inc; the bzip2 decode writes there too)
struct InflateBufs {
    DevBuf<uint8_t> d_in;
    DevBuf<uint32_t> d_cand; // the count, the candidates, the piece start
    HostBuf<uint32_t> h_cand;
    DevBuf<uint32_t> d_bcand; // block mode: the count and the block scan's candidates (bit offsets)
    HostBuf<uint32_t> h_bcand;
    DevBuf<uint16_t> d_slots; // kInflateSlotSyms symbols a segment (block mode: kInflateBlockSlotSyms)
    DevBuf<InflateSegRes> d_res;
    HostBuf<InflateSegRes> h_res;
    DevBuf<InflateLink> d_links;
    HostBuf<InflateLink> h_links;
    DevBuf<uint32_t> d_flags;
    HostBuf<uint32_t> h_flags;
    DevBuf<uint8_t> d_win;
    DevBuf<uint8_t> d_out;
    HostBuf<uint16_t> h_bslots; // block mode, default configuration: the host workers' slots (kInflateBlockSlotSyms each)
    HostBuf<uint8_t> h_bbytes;  // and their symbols narrowed to bytes
    uint64_t cand_cap() const { return d_cand.size() - 2; }
    uint64_t bcand_cap() const { return d_bcand.size() ? d_bcand.size() - 1 : 0; }
    uint32_t nslots() const { return (uint32_t)d_res.size(); }
    uint32_t nslots(uint32_t slot_syms) const { return (uint32_t)std::min<size_t>(d_res.size(), d_slots.size() / slot_syms); }
    // bcand: room for the block scan's candidates (0: flush mode, none); host_bslots: the host workers' block slots
    hipError_t ensure(uint64_t piece, uint32_t slots, int node, uint32_t slot_syms = kInflateSlotSyms, uint64_t bcand = 0,
                      uint32_t host_bslots = 0)
    {
        const uint64_t cand = piece / 4 + 16; // (a candidate per 4 bytes at most that the launch takes; more are counted, not kept)
        hipError_t e = d_flags.reserve(4);
        if (!e) e = h_flags.reserve(4, node);
        if (!e) e = d_win.reserve(kInfWindow);
        if (!e) e = d_in.reserve(piece + 16);
        if (!e) e = d_cand.reserve(cand + 2);
        if (!e) e = h_cand.reserve(cand + 2, node);
        if (!e && bcand) e = d_bcand.reserve(bcand + 1);
        if (!e && bcand) e = h_bcand.reserve(bcand + 1, node);
        if (!e) e = d_slots.reserve((size_t)slots * slot_syms);
        if (!e) e = d_res.reserve(slots);
        if (!e) e = h_res.reserve(slots, node);
        if (!e) e = d_links.reserve(slots);
        if (!e) e = h_links.reserve(slots, node);
        if (!e && host_bslots) e = h_bslots.reserve((size_t)host_bslots * kInflateBlockSlotSyms, node);
        if (!e && host_bslots) e = h_bbytes.reserve((size_t)host_bslots * kInflateBlockSlotSyms, node);
        if (e) each(Release());
        return e;
    }
    template <class F> void each(F&& f)
    {
        f(d_in); f(d_cand); f(h_cand); f(d_bcand); f(h_bcand); f(d_slots); f(d_res); f(h_res); f(d_links); f(h_links); f(d_flags); f(h_flags);
        f(d_win); f(d_out); f(h_bslots); f(h_bbytes);
    }
};

// GPU bzip2 (unbz2.inc): the compressed piece (+16) and its candidates and their count, the candidates' slots (BWT bytes,
// then the inverse BWT's output), the T vectors, the RLE1 chunk states, the symbol stage's results and the linked blocks
struct Bzip2Bufs {
    DevBuf<uint8_t> d_in;
    DevBuf<uint64_t> d_cand;
    HostBuf<uint64_t> h_cand;
    DevBuf<uint32_t> d_count;
    HostBuf<uint32_t> h_count;
    DevBuf<uint8_t> d_slots; // kBzMaxBlock bytes a slot
    DevBuf<uint32_t> d_tt;   // kBzMaxBlock words a slot
    DevBuf<uint64_t> d_chunks; // kBzChunks a slot
    DevBuf<BzBlockRes> d_res;
    HostBuf<BzBlockRes> h_res;
    DevBuf<BzGpuBlock> d_blk;
    HostBuf<BzGpuBlock> h_blk;
    uint64_t cand_cap() const { return d_cand.size(); }
    uint32_t nslots() const { return (uint32_t)d_res.size(); }
    hipError_t ensure(uint64_t piece, uint32_t slots, int node)
    {
        const uint64_t cand = bz_candidate_cap(piece);
        hipError_t e = d_count.reserve(4);
        if (!e) e = h_count.reserve(4, node);
        if (!e) e = d_in.reserve(piece + 16);
        if (!e) e = d_cand.reserve(cand);
        if (!e) e = h_cand.reserve(cand, node);
        if (!e) e = d_slots.reserve((size_t)slots * kBzMaxBlock);
        if (!e) e = d_tt.reserve((size_t)slots * kBzMaxBlock);
        if (!e) e = d_chunks.reserve((size_t)slots * kBzChunks);
        if (!e) e = d_res.reserve(slots);
        if (!e) e = h_res.reserve(slots, node);
        if (!e) e = d_blk.reserve(slots);
        if (!e) e = h_blk.reserve(slots, node);
        if (e) each(Release());
        return e;
    }
    template <class F> void each(F&& f)
    {
        f(d_in); f(d_cand); f(h_cand); f(d_count); f(h_count); f(d_slots); f(d_tt); f(d_chunks); f(d_res); f(h_res); f(d_blk); f(h_blk);
    }
};

// CRC-32 and CRC-64/XZ of ranges in HBM (crc_kernels.hip): the ranges and the prefix of their tile counts, built in pinned memory, and
// their HBM twins; a remainder per tile; the finished CRCs and their way back
struct CrcBufs {
    Twin<uint64_t> offs, lens;
    Twin<uint32_t> tile0; // n + 1
    DevBuf<uint32_t> d_partial;
    Twin<uint32_t> crcs;
    DevBuf<uint64_t> d_partial64; // CRC-64/XZ: its remainders and results
    Twin<uint64_t> crcs64;
    template <class Crc> DevBuf<Crc>& partial()
    {
        if constexpr (sizeof(Crc) == 8) return d_partial64;
        else return d_partial;
    }
    template <class Crc> Twin<Crc>& result()
    {
        if constexpr (sizeof(Crc) == 8) return crcs64;
        else return crcs;
    }
    hipError_t ensure(size_t n, size_t tiles, size_t width) // width: the bytes of a CRC, 4 or 8
    {
        hipError_t e = offs.ensure(n);
        if (!e) e = lens.ensure(n);
        if (!e) e = tile0.ensure(n + 1);
        if (!e) e = width == 8 ? d_partial64.reserve(std::max<size_t>(tiles, 1)) : d_partial.reserve(std::max<size_t>(tiles, 1));
        if (!e) e = width == 8 ? crcs64.ensure(n) : crcs.ensure(n);
        if (e) each(Release());
        return e;
    }
    template <class F> void each(F&& f) { offs.each(f); lens.each(f); tile0.each(f); f(d_partial); crcs.each(f); f(d_partial64); crcs64.each(f); }
};

// SHA-256 of ranges in HBM (sha256_kernels.hip): the ranges in the order the waves take them, built in pinned memory, and their
// HBM twin; the digests (32 bytes a range, in the caller's order) and their way back
struct Sha256Bufs {
    Twin<Sha256Range> ranges;
    Twin<uint8_t> digests;
    hipError_t ensure(size_t n)
    {
        hipError_t e = ranges.ensure(n);
        if (!e) e = digests.ensure(n * kSha256Digest);
        if (e) each(Release());
        return e;
    }
    template <class F> void each(F&& f) { ranges.each(f); digests.each(f); }
};

// The BCJ filters over ranges in HBM (bcj_kernels.hip): the range table (n + 1 entries) built in pinned memory and its HBM twin,
// and a word a stretch for the x86 restart points
struct BcjBufs {
    Twin<BcjRange> ranges;
    DevBuf<uint32_t> d_points;
    Twin<uint32_t> tile0;     // Delta's: the ranges' first tiles, and kDeltaTail bytes a tile (ensure_delta; empty otherwise)
    DevBuf<uint8_t> d_delta;
    hipError_t ensure(size_t n, size_t units)
    {
        hipError_t e = ranges.ensure(n + 1);
        if (!e) e = d_points.reserve(std::max<size_t>(units, 1));
        if (e) each(Release());
        return e;
    }
    hipError_t ensure_delta(size_t n, size_t tiles)
    {
        hipError_t e = tile0.ensure(n + 1);
        if (!e) e = d_delta.reserve(std::max<size_t>(tiles, 1) * kDeltaTail);
        if (e) each(Release());
        return e;
    }
    template <class F> void each(F&& f) { ranges.each(f); f(d_points); tile0.each(f); f(d_delta); }
};

// GPU LZMA2 (unxz.inc): the whole .xz file and the Blocks the kernel takes
struct XzBufs {
    DevBuf<uint8_t> d_in;
    Twin<XzGpuBlock> blk;
    hipError_t ensure(uint64_t bytes, size_t nb)
    {
        hipError_t e = d_in.reserve(bytes + 16);
        if (!e) e = blk.ensure(std::max<size_t>(nb, 1));
        if (e) each(Release());
        return e;
    }
    template <class F> void each(F&& f) { f(d_in); blk.each(f); }
};

// GPU LZMA2 encoder (xzpack.inc), for a staging slot of slot_bytes: the chains and the candidates (a word per staged byte
// each: 8x the slot), the chunks' coder output, their results and final offsets, the assembled piece and its way back
struct XzEncBufs {
    DevBuf<uint32_t> d_prev, d_cand;
    DevBuf<uint8_t> d_slots, d_out;
    Twin<uint32_t> res;
    Twin<uint64_t> dst;
    HostBuf<uint8_t> h_out[2]; // double-buffered: the consumers read one while the next slot fills the other
    Twin<uint64_t> zend;       // the self-check's: where every chunk's stretch ends, and the verdicts, a chunk each: sized by
    Twin<Lzma2Verdict> chk;    // the call that asks for the check (xzpack.inc), empty otherwise
    DevBuf<uint8_t> d_filt;    // a BCJ filter's: the slot's bytes filtered, a byte per staged byte: allocated by the call that
    Twin<CmpChunk> fcmp;       // asks for a filter; with the self-check too, the range-compare kernel's table and its verdicts,
    Twin<uint8_t> feq;         // a byte a Block
    DevBuf<uint32_t> d_cand_set; // level 1's: kXzEncCands words per staged byte: allocated by the call that asks for level 1
    hipError_t ensure_level(uint64_t slot_bytes)
    {
        const hipError_t e = d_cand_set.reserve(slot_bytes * kXzEncCands);
        if (e) each(Release()); // (none of it is left behind)
        return e;
    }
    hipError_t ensure_filter(uint64_t slot_bytes) { return d_filt.reserve(slot_bytes + 16); } // (the compare kernel loads 16 bytes at a time)
    hipError_t ensure_filter_check(uint64_t slot_bytes)
    {
        const size_t nblk = (size_t)(slot_bytes / kXzEncChunk + 1); // (a Block is a chunk at least)
        hipError_t e = fcmp.ensure((size_t)(slot_bytes / kCmpChunk) + nblk);
        if (!e) e = feq.ensure(nblk);
        return e;
    }
    hipError_t ensure_check(uint64_t slot_bytes)
    {
        const size_t nch = std::max<size_t>((size_t)((slot_bytes + kXzEncChunk - 1) / kXzEncChunk), 1);
        hipError_t e = zend.ensure(nch);
        if (!e) e = chk.ensure(nch);
        return e;
    }
    // what a slot's output takes at most: every chunk stored (3 bytes of header), a Block a chunk (a header of 20 bytes
    // for sizes that take four bytes each, the end byte, 3 of padding and the longest Check, SHA-256's 32: 59 in all)
    static uint64_t out_cap(uint64_t slot_bytes) { return slot_bytes + ((slot_bytes + kXzEncChunk - 1) / kXzEncChunk) * 64 + 64; }
    uint64_t cap() const { return h_out[0].size(); }
    hipError_t ensure(uint64_t slot_bytes, int node)
    {
        const size_t nch = (size_t)((slot_bytes + kXzEncChunk - 1) / kXzEncChunk);
        hipError_t e = d_prev.reserve(slot_bytes);
        if (!e) e = d_cand.reserve(slot_bytes);
        if (!e) e = d_slots.reserve(nch * kXzEncSlot);
        if (!e) e = d_out.reserve(out_cap(slot_bytes));
        if (!e) e = res.ensure(std::max<size_t>(nch, 1));
        if (!e) e = dst.ensure(std::max<size_t>(nch, 1));
        for (HostBuf<uint8_t>& b : h_out)
            if (!e) e = b.reserve(out_cap(slot_bytes), node);
        if (e) each(Release()); // (none of it is left behind)
        return e;
    }
    template <class F> void each(F&& f) { f(d_prev); f(d_cand); f(d_slots); f(d_out); res.each(f); dst.each(f); f(h_out[0]); f(h_out[1]); zend.each(f); chk.each(f); f(d_filt); fcmp.each(f); feq.each(f); f(d_cand_set); }
};

// GPU bzip2 encoder (bzpack.inc), for `blocks` blocks a launch of up to `cap` bytes each after RLE1: the sort's scratch
// (kBzEncScratchPerByte bytes a byte), the stages' arrays, the blocks' output slots, the assembled piece and its way back.
// The dimensions the buffers were made for are kept: a call that fits them allocates nothing, any other frees all of it
// and allocates for its own (blocks x cap never exceeds kBzEncLaunchBytes: bzpack.inc), and a failure leaves none of it.
struct BzEncBufs {
    DevBuf<uint8_t> d_rle, d_last, d_sel;
    DevBuf<uint64_t> d_key_a, d_key_b;
    DevBuf<uint32_t> d_idx_a, d_idx_b, d_rank, d_slots, d_out;
    DevBuf<uint16_t> d_syms;
    DevBuf<BzEncMap> d_maps;
    Twin<BzEncJob> jobs;
    Twin<BzBwtJob> bwt_jobs;
    Twin<BzEncRes> res;
    Twin<uint64_t> dst;
    HostBuf<uint8_t> h_out[2]; // double-buffered: the consumers read one while the next slot fills the other
    Twin<Bz2CheckJob> ckjobs;  // the self-check's: every block's table entry and verdict: sized by the call that asks for
    Twin<Bz2Verdict> chk;      // the check (bzpack.inc, behind ensure, which may release them), empty otherwise
    hipError_t ensure_check(uint32_t blocks)
    {
        hipError_t e = ckjobs.ensure(std::max<size_t>(blocks, 1));
        if (!e) e = chk.ensure(std::max<size_t>(blocks, 1));
        return e;
    }
    uint32_t made_blocks = 0, made_cap = 0;
    uint64_t out_words() const { return (uint64_t)made_blocks * bzenc_slot_words(made_cap) + 2; }
    hipError_t ensure(uint32_t blocks, uint32_t cap, bool with_output, int node)
    {
        cap = (cap + 63) & ~63u;
        if (blocks <= made_blocks && cap <= made_cap) {
            if (!with_output || h_out[0].size()) return hipSuccess;
            blocks = made_blocks; // (made for snaphash_bwt_device, which takes no output buffers: they are added)
            cap = made_cap;
        } else {
            each(Release());
        }
        const size_t nb = blocks, el = (size_t)blocks * cap, room = (size_t)blocks * (cap + 64);
        hipError_t e = d_rle.reserve(room);
        if (!e) e = d_last.reserve(room);
        if (!e) e = d_syms.reserve(room);
        if (!e) e = d_key_a.reserve(el);
        if (!e) e = d_key_b.reserve(el);
        if (!e) e = d_idx_a.reserve(el);
        if (!e) e = d_idx_b.reserve(el);
        if (!e) e = d_rank.reserve(el);
        if (!e) e = d_maps.reserve(nb);
        if (!e) e = d_sel.reserve(nb * kBzEncSelStride);
        if (!e) e = jobs.ensure(nb);
        if (!e) e = bwt_jobs.ensure(nb);
        if (!e) e = res.ensure(nb);
        if (!e) e = dst.ensure(nb);
        const size_t words = nb * bzenc_slot_words(cap) + 2;
        if (!e && with_output) {
            e = d_slots.reserve(words);
            if (!e) e = d_out.reserve(words);
            for (HostBuf<uint8_t>& b : h_out)
                if (!e) e = b.reserve(words * 4, node);
        }
        if (e) {
            each(Release()); // (none of it is left behind)
            made_blocks = made_cap = 0;
            return e;
        }
        made_blocks = blocks;
        made_cap = cap;
        return hipSuccess;
    }
    BzEncScratch scratch() const
    {
        BzEncScratch s{};
        s.cap = made_cap;
        s.slot_words = bzenc_slot_words(made_cap);
        s.rle = d_rle.data(); s.last = d_last.data();
        s.key_a = d_key_a.data(); s.key_b = d_key_b.data();
        s.idx_a = d_idx_a.data(); s.idx_b = d_idx_b.data(); s.rank = d_rank.data();
        s.syms = d_syms.data(); s.maps = d_maps.data(); s.sel = d_sel.data();
        s.slots = d_slots.data(); s.bwt_jobs = bwt_jobs.d.data(); s.res = res.d.data();
        return s;
    }
    template <class F> void each(F&& f)
    {
        f(d_rle); f(d_last); f(d_sel); f(d_key_a); f(d_key_b); f(d_idx_a); f(d_idx_b); f(d_rank); f(d_slots); f(d_out); f(d_syms); f(d_maps);
        jobs.each(f); bwt_jobs.each(f); res.each(f); dst.each(f); f(h_out[0]); f(h_out[1]); ckjobs.each(f); chk.each(f);
    }
};

} // namespace snaphash
