// Host harness of the install side's block mode (snappy_amd/csrc/inflate_core.h inf_dynamic_ok and inflate_run's block
// stop rule; inflate_host.cpp), for tests/test_inflate_blocks_host.py: the scan's checker against inf_dynamic at every
// bit offset, a serial block walk that records every block, the block-stop decode of one segment, and the whole block
// mode run serially -- scan, decode of every candidate into a hole slot, link, fill, the host taking one block where the
// chain breaks -- as the library's driver (unpack.inc) runs it with the GPU kernels or host threads.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../include/snaphash.h"
#include "../snappy_amd/csrc/inflate_host.cpp"
#include "../snappy_amd/csrc/tarpack.cpp"
#include "../snappy_amd/csrc/walk.cpp"
#include "../snappy_amd/csrc/hostfill.cpp" // walk.cpp sizes its thread pools with usable_cpus()

using namespace snaphash;

extern "C" {

// what BTYPE = 2 and inf_dynamic answer from `bit`, with the header inside in[0..n)
int ibh_dynamic_ref(const uint8_t* in, size_t n, uint64_t bit)
{
    InfBits b;
    b.in = in;
    b.n = n;
    b.pos = bit >> 3;
    b.buf = 0;
    b.cnt = 0;
    ib_fill(b);
    ib_take(b, (uint32_t)(bit & 7));
    ib_fill(b);
    ib_take(b, 1);
    if (ib_take(b, 2) != 2) return 0;
    static InflateTables t;
    return inf_dynamic(b, t) && ib_consumed(b) <= (uint64_t)n * 8;
}

int ibh_dynamic_ok(const uint8_t* in, size_t n, uint64_t bit) { return inf_dynamic_ok(in, n, bit); }

// both at every bit offset of in[0..n): *accepted by the checker; mismatches counted, the first one's bit in *first
uint64_t ibh_diff(const uint8_t* in, size_t n, uint64_t* accepted, uint64_t* first)
{
    uint64_t bad = 0, acc = 0;
    *first = ~0ull;
    for (uint64_t bit = 0; bit < (uint64_t)n * 8; ++bit) {
        const int a = inf_dynamic_ok(in, n, bit), r = ibh_dynamic_ref(in, n, bit);
        acc += a;
        if (a != r) {
            if (!bad) *first = bit;
            ++bad;
        }
    }
    *accepted = acc;
    return bad;
}

// the checker's candidates in in[0..n), ascending; returns how many there are, writes at most cap
size_t ibh_scan(const uint8_t* in, size_t n, uint64_t* out, size_t cap)
{
    size_t k = 0;
    for (uint64_t bit = 0; bit < (uint64_t)n * 8; ++bit)
        if (inf_dynamic_ok(in, n, bit)) {
            if (k < cap) out[k] = bit;
            ++k;
        }
    return k;
}

// A serial walk of the raw DEFLATE stream in[0..n) that records each block: start bit, BTYPE, output bytes (and the
// first bit after the final block in *end).  Returns the number of blocks (at most cap written), -1 if the stream is bad.
long ibh_blocks(const uint8_t* in, size_t n, uint64_t* start, uint32_t* type, uint64_t* out_len, size_t cap, uint64_t* end)
{
    const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    const uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    const uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    static InflateTables t;
    InfBits b;
    b.in = in;
    b.n = n;
    b.pos = 0;
    b.buf = 0;
    b.cnt = 0;
    long k = 0;
    for (;;) {
        ib_fill(b);
        const uint64_t s0 = ib_consumed(b);
        const uint32_t final = ib_take(b, 1), ty = ib_take(b, 2);
        uint64_t o = 0;
        if (ty == 0) {
            ib_take(b, b.cnt & 7);
            const uint64_t at = ib_consumed(b) >> 3;
            if (at + 4 > n) return -1;
            const uint32_t len = in[at] | (uint32_t)in[at + 1] << 8;
            o = len;
            b.pos = at + 4 + len;
            b.buf = 0;
            b.cnt = 0;
            if (b.pos > n) return -1;
        } else {
            if (ty == 1) inf_fixed(t);
            else if (ty != 2 || !inf_dynamic(b, t)) return -1;
            for (;;) {
                ib_fill(b);
                const int32_t s = inf_decode(b, t.lit);
                if (s < 0 || ib_over(b)) return -1;
                if (s < 256) { ++o; continue; }
                if (s == 256) break;
                if (s > 285) return -1;
                o += lbase[s - 257] + ib_take(b, lext[s - 257]);
                const int32_t ds = inf_decode(b, t.dist);
                if (ds < 0 || ds > 29) return -1;
                ib_take(b, dext[ds]);
            }
        }
        if ((size_t)k < cap) {
            start[k] = s0;
            type[k] = ty;
            out_len[k] = o;
        }
        ++k;
        if (final) {
            ib_fill(b);
            *end = ib_consumed(b);
            return k;
        }
    }
}

// one segment in block mode with holes: status, cut, end bit, output symbols and hole_end
int ibh_segment(const uint8_t* in, size_t n, uint64_t start_bit, size_t cap, uint64_t block_min, int* cut, uint64_t* end_bit,
                uint64_t* out_len, uint32_t* hole_end)
{
    static InflateTables t;
    std::vector<uint16_t> seg(cap + 1);
    const InflateRun r = inflate_run<uint16_t>(in, n, start_bit, seg.data(), 0, cap, true, false, t, block_min);
    *cut = r.cut;
    *end_bit = r.end_bit;
    *out_len = r.out_len;
    *hole_end = r.hole_end;
    return r.status;
}

struct BlockStats {
    uint64_t pieces, candidates, linked, linked_from_block, host_blocks, host_bytes;
};

// The block mode, serially, on every member of gz[0..n): pieces of at most `piece` compressed bytes starting at any bit,
// candidates = the checker's block starts + stored-block ends + the piece's start, each decoded on its own into a slot of
// slot_syms symbols (block_min as inflate_run), the chain linked from the piece's start and filled in order; where it
// breaks at the piece's start, the host decoder takes one block.  0 or SNAPHASH_EFORMAT.
int ibh_gunzip_blocks(const uint8_t* gz, size_t n, size_t piece, uint32_t slot_syms, uint64_t block_min, uint8_t** out_p,
                      size_t* out_len, BlockStats* st)
{
    memset(st, 0, sizeof *st);
    std::vector<uint8_t> out;
    *out_p = nullptr;
    *out_len = 0;
    InflateTables t;
    size_t at = 0;
    int rc = n ? 0 : SNAPHASH_EFORMAT;
    while (!rc && at < n) {
        size_t h = 0;
        if (gzip_header(gz + at, n - at, &h)) { rc = SNAPHASH_EFORMAT; break; }
        const uint8_t* z = gz + at + h;
        const uint64_t zn = n - at - h;
        const size_t m0 = out.size();
        uint64_t cur = 0, final_bit = 0; // bit cursor in z
        bool ended = false;
        while (!ended && !rc) {
            const uint64_t b0 = cur >> 3, sb = cur & 7, pn = std::min<uint64_t>(piece, zn - b0);
            const uint8_t* p = z + b0;
            std::vector<uint64_t> cand;
            for (uint64_t bit = 0; bit < pn * 8; ++bit)
                if (inf_dynamic_ok(p, pn, bit)) cand.push_back(bit);
            st->candidates += cand.size();
            const size_t nb = cand.size();
            for (uint64_t v : flush_candidates(p, pn)) cand.push_back(v * 8);
            cand.push_back(sb);
            std::vector<uint64_t> blocks(cand.begin(), cand.begin() + nb);
            std::sort(cand.begin(), cand.end());
            cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
            ++st->pieces;
            std::vector<std::vector<uint16_t>> slot(cand.size());
            std::vector<InflateRun> res(cand.size());
            for (size_t i = 0; i < cand.size(); ++i) {
                if (cand[i] < sb) continue;
                slot[i].resize(slot_syms);
                res[i] = inflate_run<uint16_t>(p, pn, cand[i], slot[i].data(), 0, slot_syms, true, false, t, block_min);
            }
            uint64_t pos = sb, nl = 0;
            for (;;) {
                const auto it = std::lower_bound(cand.begin(), cand.end(), pos);
                if (it == cand.end() || *it != pos) break;
                const size_t i = (size_t)(it - cand.begin());
                const InflateRun& r = res[i];
                if (r.status != kInfBlock && r.status != kInfFinal) break;
                const size_t base = out.size();
                out.resize(base + (size_t)r.out_len);
                for (uint64_t q = r.hole_end; q < r.out_len; ++q)
                    if (slot[i][q] >= kInfHole) { rc = SNAPHASH_EFORMAT; break; } // (hole_end must cover every hole)
                if (rc || !fill_holes_host(slot[i].data(), (size_t)r.out_len, out.data() + base, base - m0)) { rc = SNAPHASH_EFORMAT; break; }
                ++nl;
                if (std::binary_search(blocks.begin(), blocks.end(), pos)) ++st->linked_from_block;
                if (r.status == kInfFinal) { ended = true; final_bit = b0 * 8 + r.end_bit; break; }
                pos = r.end_bit;
                if (pos >= pn * 8) break;
            }
            if (rc) break;
            st->linked += nl;
            if (nl) { cur = b0 * 8 + pos; continue; }
            // the chain breaks at the piece's start: one block on the host
            const size_t o0 = out.size();
            const InflateRun r = inflate_host_append(z, zn, cur, out, m0, false, 0);
            ++st->host_blocks;
            st->host_bytes += out.size() - o0;
            if (r.status == kInfFinal) { ended = true; final_bit = r.end_bit; }
            else if (r.status == kInfBlock && r.end_bit > cur) cur = r.end_bit;
            else rc = SNAPHASH_EFORMAT;
        }
        if (rc) break;
        const uint32_t crc = crc32_update(0, out.data() + m0, out.size() - m0);
        size_t next = 0;
        if (gzip_trailer(z, zn, final_bit, crc, out.size() - m0, &next)) { rc = SNAPHASH_EFORMAT; break; }
        at += h + next;
    }
    if (rc) return rc;
    *out_p = (uint8_t*)malloc(out.size() + 1);
    if (!out.empty()) memcpy(*out_p, out.data(), out.size());
    *out_len = out.size();
    return 0;
}

void ibh_free(void* p) { free(p); }

} // extern "C"
