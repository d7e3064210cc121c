// lzma2_check_host_harness.cpp -- the .xz producer's self-check (snappy_amd/csrc/lzma2_check_core.h, the walk
// lzma2_check_kernel runs) compiled for the host, for tests/test_lzma2_check_host.py and tests/test_gpu_lzma2_check_edges.py:
// the walker over a table of chunks, the producer's host model (xz_enc_core.h) as chunks in place with the two tables the
// producer's host side derives, and the words of a refusal.
#include <stdlib.h>
#include <string.h>

#include "../snappy_amd/csrc/lzma2_check_core.h"
#include "../snappy_amd/csrc/xz_enc_core.h"

using namespace snaphash;

static_assert(kLzCheckChunk == kXzEncChunk && kLzCheckProbs == kXzEncProbs && kLzCheckProps == kXzEncProps, "the check walks what the producer writes");

extern "C" {

// every chunk of in[0 .. n_in) (Blocks of bs bytes) against its stretch [z_beg[c], z_end[c]) of z[0 .. n_z): verdicts[2c] the
// status, verdicts[2c + 1] the offset
void lc_check(const uint8_t* in, size_t n_in, uint64_t bs, const uint8_t* z, size_t n_z, const uint64_t* z_beg, const uint64_t* z_end, size_t nch,
              uint32_t* verdicts)
{
    std::vector<uint16_t> probs(kLzCheckProbs);
    for (size_t c = 0; c < nch; ++c) {
        const Lzma2Verdict v = lzma2_check_chunk(in, n_in, bs, z, n_z, z_beg[c], z_end[c], (uint32_t)c, probs.data());
        verdicts[2 * c] = v.status;
        verdicts[2 * c + 1] = v.offset;
    }
}

// The host model of the producer over p[0 .. n), Blocks of block_size bytes: the Blocks one after another in out (chunk
// headers, bodies and end bytes over what the caller put there; Block headers, padding and Checks are not written), z_beg
// the chunks' places and z_end their stretches' ends as xzpack.inc derives them (lzma2_check_stretch_end).  Returns the
// bytes of out the Blocks take, or -1 (a refused block size, out_cap too small).
int64_t lc_encode(const uint8_t* p, size_t n, uint64_t block_size, uint8_t* out, size_t out_cap, uint64_t* z_beg, uint64_t* z_end)
{
    if (!xzenc_block_size(&block_size)) return -1;
    std::vector<uint32_t> head(1u << kXzEncHashBits), prev, cand, res;
    std::vector<uint16_t> probs(kXzEncProbs);
    std::vector<uint8_t> slots;
    NoEncOps ops;
    uint64_t at = 0;
    uint32_t ch0 = 0;
    for (uint64_t b0 = 0; b0 < n; b0 += block_size) {
        const uint32_t blen = (uint32_t)std::min<uint64_t>(block_size, n - b0);
        const uint32_t nch = (blen + kXzEncChunk - 1) / kXzEncChunk;
        prev.resize(blen);
        cand.resize(blen);
        res.resize(nch);
        slots.resize((size_t)nch * kXzEncSlot);
        const XzEncBlockLayout L = xzenc_block_stages(p + b0, blen, prev.data(), cand.data(), head.data(), probs.data(), res.data(), z_beg + ch0,
                                                      slots.data(), ops);
        if (at + L.total > out_cap) return -1;
        xzenc_block_place(p + b0, blen, res.data(), z_beg + ch0, slots.data(), out + at);
        for (uint32_t i = 0; i < nch; ++i) z_beg[ch0 + i] += at;
        for (uint32_t i = 0; i < nch; ++i) z_end[ch0 + i] = lzma2_check_stretch_end(z_beg + ch0, i, nch, at + L.hdr + L.data);
        at += L.total;
        ch0 += nch;
    }
    return (int64_t)at;
}

// last_error's words for a refused chunk, into buf (cap bytes, terminated): the length the text has
size_t lc_error_text(const char* member, uint64_t block, uint64_t chunk, uint32_t status, uint64_t at, char* buf, size_t cap)
{
    const std::string s = lzma2_check_error_text(member, block, chunk, status, at);
    if (cap) {
        const size_t k = s.size() < cap - 1 ? s.size() : cap - 1;
        memcpy(buf, s.data(), k);
        buf[k] = 0;
    }
    return s.size();
}

} // extern "C"
