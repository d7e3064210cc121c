// xzfilt_host_harness.cpp -- the .xz filters' shared headers (snappy_amd/csrc/bcj_core.h, delta_core.h) compiled for the host,
// for tests/test_xzfilt_host.py, tests/asan_xzfilt.cpp (which includes this file) and the GPU tests of the filters: a Block
// filtered on one thread, the word filters' cut run stretch by stretch, and Delta's kernels modelled tile by tile and lane by
// lane from the pieces delta_kernels.hip runs; and with the host decoder (xz_host.cpp) xz_plan's view of a file in each of its
// three chain modes, a whole file decoded, and the producer's host model (xz_enc_core.h) with a chain.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../snappy_amd/csrc/xz_host.cpp"
#include "../snappy_amd/csrc/xz_enc_core.h"

using namespace snaphash;

// Delta's decode as the three kernels run it, with tiles of `tile` bytes and workgroups of `lanes` lanes (d <= lanes): every
// tile's column sums, every column's carries, then every tile's running sums -- the tiles in descending order (order != 0)
// or ascending, to show that no tile depends on another's writes.
static void delta_decode_tiles(uint8_t* b, uint64_t len, uint32_t d, uint64_t tile, uint32_t lanes, int order)
{
    const uint64_t nt = (len + tile - 1) / tile;
    std::vector<uint8_t> scratch(nt * kDeltaTail + 1), part(lanes);
    for (uint64_t t = 0; t < nt; ++t) { // delta_sums_kernel
        const uint64_t s = t * tile, e = s + tile < len ? s + tile : len;
        for (uint32_t lane = 0; lane < lanes; ++lane) part[lane] = delta_lane_sum(b, s, e, d, delta_lane(s, e, d, lanes, lane));
        for (uint32_t c = 0; c < d; ++c) scratch[t * kDeltaTail + c] = delta_tile_total(part.data(), d, lanes, c);
    }
    for (uint32_t c = 0; c < d; ++c) delta_carry_column(scratch.data(), nt, kDeltaTail, c); // delta_carry_kernel
    for (uint64_t k = 0; k < nt; ++k) { // delta_apply_kernel
        const uint64_t t = order ? nt - 1 - k : k, s = t * tile, e = s + tile < len ? s + tile : len;
        for (uint32_t lane = 0; lane < lanes; ++lane) part[lane] = delta_lane_sum(b, s, e, d, delta_lane(s, e, d, lanes, lane));
        for (uint32_t q = 0; q < lanes; ++q) { // (the lanes in descending order too: a lane reads no byte another writes)
            const uint32_t lane = order ? lanes - 1 - q : q;
            const DeltaLane L = delta_lane(s, e, d, lanes, lane);
            if (L.ra == L.rb) continue;
            delta_lane_apply(b, s, e, d, L, delta_lane_seed(part.data(), d, lane, scratch[t * kDeltaTail + L.c]));
        }
    }
}

// Delta's encode as the two kernels run it: every whole tile's tail, then every tile from its end in slabs of lanes x
// kDeltaSlab bytes, a slab read whole before it is written.
static void delta_encode_tiles(uint8_t* b, uint64_t len, uint32_t d, uint64_t tile, uint32_t lanes, int order)
{
    const uint64_t nt = (len + tile - 1) / tile, slab = (uint64_t)lanes * kDeltaSlab;
    std::vector<uint8_t> scratch(nt * kDeltaTail + 1), out(slab);
    for (uint64_t t = 0; t < nt; ++t) { // delta_tails_kernel
        const uint64_t s = t * tile, e = s + tile < len ? s + tile : len;
        if (e - s < tile) continue;
        for (uint32_t k = 0; k < kDeltaTail; ++k) scratch[t * kDeltaTail + k] = delta_tail_byte(b, e, k);
    }
    for (uint64_t q = 0; q < nt; ++q) { // delta_encode_kernel
        const uint64_t t = order ? nt - 1 - q : q, s = t * tile, e = s + tile < len ? s + tile : len;
        const uint8_t* tail = scratch.data() + (t ? t - 1 : 0) * kDeltaTail;
        for (uint64_t k = (e - s + slab - 1) / slab; k-- > 0;) {
            const uint64_t i0 = s + k * slab;
            for (uint64_t j = 0; j < slab && i0 + j < e; ++j) out[j] = (uint8_t)(b[i0 + j] - delta_byte_in_front(b, i0 + j, d, s, tail));
            for (uint64_t j = 0; j < slab && i0 + j < e; ++j) b[i0 + j] = out[j];
        }
    }
}

extern "C" {

// bcj_block (ids 4 .. 9) or delta_block (id 3, param: the distance) in place; -1 for arguments the library refuses
int xf_block(uint32_t id, uint32_t param, int encode, uint8_t* b, size_t len, uint32_t start)
{
    if (id == kXzDelta) {
        if (!delta_dist_valid(param) || start) return -1;
        delta_block(encode != 0, b, len, param);
        return 0;
    }
    if (!xz_filter_valid(id) || param || (start & (bcj_alignment(id) - 1))) return -1;
    bcj_block(id, encode != 0, b, len, start);
    return 0;
}

// a word filter's share of every stretch (bcj_stretch_apply, what bcj_apply_kernel runs a lane a stretch), the stretches in
// descending order (order != 0) or ascending.  stretch: a multiple of 16
void xf_cut(uint32_t id, int encode, uint8_t* b, size_t len, uint32_t start, uint32_t stretch, int order)
{
    const uint64_t nk = (len + stretch - 1) / stretch;
    for (uint64_t i = 0; i < nk; ++i) bcj_stretch_apply(id, encode != 0, b, len, order ? nk - 1 - i : i, nk, stretch, nullptr, start);
}

// Delta as the kernels run it
void xf_delta_tiles(int encode, uint8_t* b, size_t len, uint32_t d, uint64_t tile, uint32_t lanes, int order)
{
    if (encode) delta_encode_tiles(b, len, d, tile, lanes, order);
    else delta_decode_tiles(b, len, d, tile, lanes, order);
}

uint32_t xf_alignment(uint32_t id) { return bcj_alignment(id); }

// xz_plan with chains = 0 (one LZMA2), 1 (or one of x86 / ARM / Thumb in front) or 2 (any chain): its verdict, the Blocks'
// count, and for the first `cap` Blocks nfilt[i], ids[3 i ..], params[3 i ..], bcj[i]; why[0 .. 128): the text
int xf_plan(const uint8_t* p, size_t n, int chains, uint64_t* nblocks, uint32_t* nfilt, uint32_t* ids, uint32_t* params, uint32_t* bcj, size_t cap,
            char* why)
{
    std::vector<XzBlock> blocks;
    uint64_t total = 0;
    std::string w;
    const int e = xz_plan(p, n, blocks, &total, w, chains);
    *nblocks = blocks.size();
    for (size_t i = 0; i < blocks.size() && i < cap; ++i) {
        nfilt[i] = blocks[i].nfilt;
        bcj[i] = blocks[i].bcj;
        for (int k = 0; k < 3; ++k) {
            ids[3 * i + k] = blocks[i].filt[k];
            params[3 * i + k] = blocks[i].fparam[k];
        }
    }
    snprintf(why, 128, "%s", w.c_str());
    return e;
}

void* xf_decode(const uint8_t* p, size_t n, unsigned threads, int chains, size_t* out_len, int* rc)
{
    std::vector<uint8_t> out;
    std::string why;
    *rc = xz_decode_host(p, n, out, threads, nullptr, why, chains);
    *out_len = *rc ? 0 : out.size();
    void* q = malloc(out.size() ? out.size() : 1);
    if (*out_len) memcpy(q, out.data(), out.size());
    return q;
}

// the producer's host model with Check CRC-64 and a chain of chain_len words, id | param << 8 as snaphash_xz_options.chain
// holds them: a malloc'ed .xz file, or *rc = -1 for a block size or a chain outside the format decisions
void* xf_encode(const uint8_t* p, size_t n, uint64_t block_size, uint32_t chain_len, const uint32_t* chain, size_t* out_len, int* rc)
{
    std::vector<uint8_t> out;
    NoEncOps ops;
    XzEncChain ch;
    ch.n = chain_len;
    for (uint32_t k = 0; k < 3 && k < chain_len; ++k) {
        ch.id[k] = chain[k] & 0xff;
        ch.param[k] = chain[k] >> 8;
    }
    *rc = xzenc_host(p, n, block_size, (uint32_t)kXzCheckCrc64, out, ops, [](const uint8_t* q, uint64_t len, uint8_t* f) { xzenc_le64(f, xz_crc64(q, len)); },
                     nullptr, ch)
              ? 0
              : -1;
    *out_len = *rc ? 0 : out.size();
    void* q = malloc(*out_len ? *out_len : 1);
    if (*out_len) memcpy(q, out.data(), *out_len);
    return q;
}

void xf_free(void* p) { free(p); }

} // extern "C"
