// bcj_host_harness.cpp -- the BCJ filters' shared header (snappy_amd/csrc/bcj_core.h) compiled for the host, with the host
// decoder (xz_host.cpp) and the producer's host model (xz_enc_core.h) that use it, for tests/test_bcj_host.py and the GPU
// tests of the filters: a Block filtered on one thread, the kernels' cut run stretch by stretch, xz_plan's view of a file
// with and without the BCJ chains allowed, a whole file decoded, and the model's file with a filter.
#include <stdlib.h>
#include <string.h>

#include "../snappy_amd/csrc/xz_host.cpp"
#include "../snappy_amd/csrc/xz_enc_core.h"

using namespace snaphash;

extern "C" {

// bcj_block in place
void bh_block(uint32_t filter, int encode, uint8_t* b, size_t len, uint32_t start) { bcj_block(filter, encode != 0, b, len, start); }

// The kernels' two passes over b[0 .. len) as one Block, a stretch at a time: every stretch's first restart point, then
// every stretch's share -- the stretches in descending order (order != 0) or ascending, to show that no stretch depends on
// another's writes.  points: scratch of ceil(len / stretch) words.
void bh_cut(uint32_t filter, int encode, uint8_t* b, size_t len, uint32_t start, uint32_t stretch, int order, uint32_t* points)
{
    const uint64_t nk = (len + stretch - 1) / stretch;
    if (filter == kBcjX86)
        for (uint64_t k = 0; k < nk; ++k) points[k] = bcj_x86_stretch_point(b, len, k, stretch);
    for (uint64_t i = 0; i < nk; ++i) bcj_stretch_apply(filter, encode != 0, b, len, order ? nk - 1 - i : i, nk, stretch, points, start);
}

// xz_plan: its verdict (kXzPlanOk / Format / Unsupported), the Blocks' count, and for the first `cap` Blocks their filter and
// start_offset; why[0 .. 128): the text
int bh_plan(const uint8_t* p, size_t n, int allow_bcj, uint64_t* nblocks, uint32_t* bcj, uint32_t* starts, size_t cap, char* why)
{
    std::vector<XzBlock> blocks;
    uint64_t total = 0;
    std::string w;
    const int e = xz_plan(p, n, blocks, &total, w, allow_bcj != 0);
    *nblocks = blocks.size();
    for (size_t i = 0; i < blocks.size() && i < cap; ++i) {
        bcj[i] = blocks[i].bcj;
        starts[i] = blocks[i].bcj_start;
    }
    snprintf(why, 128, "%s", w.c_str());
    return e;
}

void* bh_decode(const uint8_t* p, size_t n, unsigned threads, int allow_bcj, size_t* out_len, int* rc)
{
    std::vector<uint8_t> out;
    std::string why;
    *rc = xz_decode_host(p, n, out, threads, nullptr, why, allow_bcj != 0);
    *out_len = *rc ? 0 : out.size();
    void* q = malloc(out.size() ? out.size() : 1);
    if (*out_len) memcpy(q, out.data(), out.size());
    return q;
}

// the producer's host model with Check CRC-64 and a filter (0: none): a malloc'ed .xz file, or *rc = -1 for a block size or
// a filter outside the format decisions
void* bh_encode(const uint8_t* p, size_t n, uint64_t block_size, uint32_t filter, size_t* out_len, int* rc)
{
    std::vector<uint8_t> out;
    NoEncOps ops;
    *rc = xzenc_host(p, n, block_size, (uint32_t)kXzCheckCrc64, out, ops, [](const uint8_t* q, uint64_t len, uint8_t* f) { xzenc_le64(f, xz_crc64(q, len)); },
                     nullptr, filter)
              ? 0
              : -1;
    *out_len = *rc ? 0 : out.size();
    void* q = malloc(*out_len ? *out_len : 1);
    if (*out_len) memcpy(q, out.data(), *out_len);
    return q;
}

void bh_free(void* p) { free(p); }

} // extern "C"
