// bz2_check_host_harness.cpp -- the .bz2 producer's self-check (snappy_amd/csrc/bz2_check_core.h: the host model
// bz2_check_block, which the kernels of bz2_check_kernels.hip must agree with bit for bit) compiled for the host, for
// tests/test_bz2_check_host.py and tests/test_gpu_bz2_check_edges.py: the check over a table of blocks, the producer's host
// model (bzip2_enc_core.h) as a stream, the install side's host scan for block starts, bzip2's CRC, and the words of a refusal.
#include <stdlib.h>
#include <string.h>

#include "../include/snaphash.h"
#include "../snappy_amd/csrc/bzip2_host.cpp"
#include "../snappy_amd/csrc/bz2_check_core.h"
#include "../snappy_amd/csrc/bzip2_enc_core.h"

using namespace snaphash;

extern "C" {

// block k of the table against its piece: verdicts[2k] the status, verdicts[2k + 1] the offset
void bc_check(const uint8_t* z, size_t n_z, const uint64_t* z_beg, const uint64_t* z_end, const uint8_t* in, size_t n_in, const uint64_t* in_off,
              const uint64_t* in_len, const uint32_t* crc, uint32_t level, size_t nb, uint32_t* verdicts)
{
    BzScratch s;
    for (size_t k = 0; k < nb; ++k) {
        const Bz2CheckJob j = {z_beg[k], z_end[k], in_off[k], in_len[k], crc[k], 0};
        const Bz2Verdict v = bz2_check_block(z, n_z, in, n_in, j, level, s);
        verdicts[2 * k] = v.status;
        verdicts[2 * k + 1] = v.offset;
    }
}

// the producer's host model: the stream of data[0..n) at `level`
void* bc_encode(const uint8_t* data, size_t n, uint32_t level, size_t* len)
{
    const std::vector<uint8_t> z = bzenc_stream_host(data, n, level, nullptr);
    void* p = malloc(z.size() ? z.size() : 1);
    memcpy(p, z.data(), z.size());
    *len = z.size();
    return p;
}
void bc_free(void* p) { free(p); }

// the install side's host scan: bit offsets of every block magic in z[0..n), ascending; returns how many there are
uint64_t bc_scan(const uint8_t* z, size_t n, uint64_t* out, size_t cap)
{
    std::vector<uint64_t> c;
    const uint64_t all = bz_candidates(z, n, cap, 1, c);
    for (size_t i = 0; i < c.size() && i < cap; ++i) out[i] = c[i];
    return all;
}

uint32_t bc_crc(const uint8_t* p, size_t n) { return bz_crc_block(p, n); }
uint32_t bc_piece(uint32_t level) { return bzenc_piece(level); }

// last_error's words for a refused block, into buf (cap bytes, terminated): the length the text has
size_t bc_error_text(const char* member, uint64_t block, uint32_t status, uint64_t at, char* buf, size_t cap)
{
    const std::string s = bz2_check_error_text(member, block, status, at);
    if (cap) {
        const size_t k = s.size() < cap - 1 ? s.size() : cap - 1;
        memcpy(buf, s.data(), k);
        buf[k] = 0;
    }
    return s.size();
}

} // extern "C"
