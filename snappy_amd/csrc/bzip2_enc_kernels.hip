// bzip2_enc_kernels.hip -- the GPU bzip2 encoder of the data.tar.bz2 producer.  A bzip2 block needs nothing from any other
// block, and bzip2_enc_core.h cuts blocks by input size, so every stage runs the slot's blocks side by side, a workgroup
// (or a wave) a block:
//   rle1    1024 lanes a piece: run starts from neighbour compares, a byte's place in its run by a max-scan of the starts,
//           what it emits (bzenc_rle1_emits; a fourth byte counts the equal bytes behind it, at most 255 compares), an
//           exclusive scan for the offsets.  LDS: 128 bytes.
//   bwt     1024 lanes a block: the cyclic rotations sorted by prefix doubling.  Keys are the first four bytes, then
//           (rank[i], rank[(i + k) mod n]) with k = 4, 8, ...; every round sorts (key, index) pairs by LSD radix passes of 8
//           bits -- each wave owns a contiguous sixteenth, counts its digits in LDS, and scatters 64 at a time in order,
//           equal digits ranked among the wave's lanes with eight ballots (bz_ibwt_kernel's scatter) -- then takes the new
//           dense ranks from the key-changed flags by a scan.  Stable passes keep equal keys in start-index order.  Ends
//           when all ranks differ or k >= n: at most 22 rounds whatever the data.  LDS: 16 KiB + 128 bytes (a CU holds two workgroups: 32 waves).
//   mtf     one wave a block: the 256-entry list four to a lane, the position by a byte compare and a ballot, the shift by
//           one DPP wave shift (positions 1-3: lane 0's word in scalar registers); RUNA/RUNB for runs of the front byte
//           (bzenc_put_run_to).  LDS: the symbol map, 516 bytes; a workgroup is one wave, so a CU holds 32 of them.
//   code    1024 lanes a block: frequencies by LDS atomics, libbz2's partition on lane 0, four rounds of (a lane a group
//           of 50: cheapest table; a wave a table: code lengths), group bit lengths, a scan, the header by lane 0, then
//           every lane writes its groups MSB first.  LDS: 44 KiB (a CU holds two workgroups: 32 waves).
//   concat  shifts the blocks together at bit granularity (v_alignbit on word pairs): 256 lanes, eight workgroups a block,
//           no LDS; a CU holds eight workgroups (32 waves).
// Integer work with data-dependent control flow: no MFMA.  Every index was produced here from bounded values (ranks < n,
// MTF positions < 256, selectors < 6), and every store is checked against its buffer's end all the same.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bzip2_enc_core.h"
#include "bzip2_enc_kernels.h"

namespace snaphash {

namespace {

template <bool kMax> __device__ inline uint32_t scan_op(uint32_t a, uint32_t b) { return kMax ? (a > b ? a : b) : a + b; }

// Inclusive scan (sum, or maximum) over the workgroup's 1024 lanes; *total: over all of them.  tmp: 16 words of LDS.
// Every lane calls it.
template <bool kMax> __device__ inline uint32_t block_scan(uint32_t v, uint32_t* tmp, uint32_t* total)
{
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d);
        if (lane >= d) v = scan_op<kMax>(v, t);
    }
    __syncthreads(); // (whoever still reads tmp from the scan before)
    if (lane == 63) tmp[w] = v;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
    for (uint32_t k = 0; k < 16; ++k) {
        const uint32_t t = tmp[k];
        if (k < w) pre = scan_op<kMax>(pre, t);
        tot = scan_op<kMax>(tot, t);
    }
    *total = tot;
    return scan_op<kMax>(v, pre);
}

__global__ void __launch_bounds__(1024) bz_enc_rle1_kernel(const uint8_t* __restrict__ d_in, const BzEncJob* __restrict__ jobs, BzEncScratch s)
{
    __shared__ uint32_t tmp[16];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const uint8_t* in = d_in + jobs[b].in_off;
    const uint32_t n = jobs[b].in_len;
    const uint32_t room = s.cap + 64;
    uint8_t* out = s.rle + (uint64_t)b * room;
    uint32_t start_carry = 0, out_carry = 0, over = 0;
    for (uint32_t base = 0; base < n; base += 1024) {
        const uint32_t i = base + tid;
        const bool valid = i < n;
        const uint32_t c = valid ? in[i] : 0u;
        const bool first = valid && (i == 0 || in[i - 1] != c);
        uint32_t tot;
        uint32_t start = block_scan<true>(first ? i : 0u, tmp, &tot);
        start = max(start, start_carry);
        start_carry = max(start_carry, tot);
        const uint32_t e = valid ? bzenc_rle1_emits(i - start) : 0u;
        uint32_t behind = 0;
        if (e == 2)
            while (behind < 255 && i + 1 + behind < n && in[i + 1 + behind] == c) ++behind;
        const uint32_t o = out_carry + block_scan<false>(e, tmp, &tot) - e;
        out_carry += tot;
        if (e) {
            if (o + e <= room) {
                out[o] = (uint8_t)c;
                if (e == 2) out[o + 1] = (uint8_t)behind;
            } else {
                over = 1;
            }
        }
    }
    if (over) atomicOr(&s.res[b].over, 1u);
    if (tid == 0) {
        const uint32_t rn = out_carry <= s.cap ? out_carry : 0u; // (bzenc_rle_cap: never more)
        if (out_carry > s.cap) atomicOr(&s.res[b].over, 1u);
        s.res[b].rle_n = rn;
        s.bwt_jobs[b] = BzBwtJob{(uint64_t)b * room, (uint64_t)b * room, rn, 0};
    }
}

// One stable LSD pass over digit (key >> shift) & 255 of n (key, index) pairs, from (ka, ia) to (kb, ib).
__device__ inline void radix_pass(const uint64_t* ka, const uint32_t* ia, uint64_t* kb, uint32_t* ib, uint32_t n, uint32_t shift, uint32_t* hist,
                                  uint32_t* tmp)
{
    const uint32_t tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const uint32_t seg = ((n + 15) / 16 + 63) & ~63u; // each wave owns a contiguous sixteenth, whole 64s
    const uint32_t a = min(n, w * seg), e = min(n, (w + 1) * seg);
    for (uint32_t i = tid; i < 4096; i += 1024) hist[i] = 0;
    __syncthreads();
    for (uint32_t i = a + lane; i < e; i += 64) atomicAdd(&hist[((uint32_t)(ka[i] >> shift) & 255u) * 16 + w], 1u);
    __syncthreads();
    { // exclusive scan of hist in (digit, wave) order: where each wave's first key of each digit goes
        const uint32_t v0 = hist[tid * 4], v1 = hist[tid * 4 + 1], v2 = hist[tid * 4 + 2], v3 = hist[tid * 4 + 3];
        uint32_t tot;
        const uint32_t sum = v0 + v1 + v2 + v3;
        const uint32_t ex = block_scan<false>(sum, tmp, &tot) - sum;
        hist[tid * 4] = ex;
        hist[tid * 4 + 1] = ex + v0;
        hist[tid * 4 + 2] = ex + v0 + v1;
        hist[tid * 4 + 3] = ex + v0 + v1 + v2;
    }
    __syncthreads();
    for (uint32_t base = a; base < e; base += 64) {
        const uint32_t i = base + lane;
        const bool valid = i < e;
        const uint64_t key = valid ? ka[i] : 0;
        const uint32_t idx = valid ? ia[i] : 0;
        const uint32_t c = (uint32_t)(key >> shift) & 255u;
        uint64_t peers = __ballot(valid);
        for (uint32_t bit = 0; bit < 8; ++bit) {
            const bool on = (c >> bit) & 1u;
            const uint64_t m = __ballot(on);
            peers &= on ? m : ~m;
        }
        const uint32_t at = hist[c * 16 + w]; // (every lane reads before the group's first lane moves it on)
        if (valid) {
            const uint32_t j = at + (uint32_t)__popcll(peers & ((1ull << lane) - 1));
            if (j < n) {
                kb[j] = key;
                ib[j] = idx;
            }
            if (lane == (uint32_t)(__ffsll((long long)peers) - 1)) hist[c * 16 + w] = at + (uint32_t)__popcll(peers);
        }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(1024) bz_enc_bwt_kernel(const uint8_t* __restrict__ d_in, const BzBwtJob* __restrict__ jobs, uint8_t* d_out,
                                                          uint32_t* d_op, uint32_t op_stride, BzEncScratch s)
{
    __shared__ uint32_t hist[4096];
    __shared__ uint32_t tmp[16];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const uint32_t n = jobs[b].n;
    if (n == 0 || n > s.cap) { // (the launchers pass no such range)
        if (tid == 0) d_op[(uint64_t)b * op_stride] = 0;
        return;
    }
    const uint8_t* in = d_in + jobs[b].in_off;
    uint8_t* out = d_out + jobs[b].out_off;
    uint64_t *ka = s.key_a + (uint64_t)b * s.cap, *kb = s.key_b + (uint64_t)b * s.cap;
    uint32_t *ia = s.idx_a + (uint64_t)b * s.cap, *ib = s.idx_b + (uint64_t)b * s.cap;
    uint32_t* rank = s.rank + (uint64_t)b * s.cap;
    uint32_t rbits = 1; // bits of a rank (< n)
    while (rbits < 20 && (1u << rbits) < n) ++rbits;
    for (uint32_t i = tid; i < n; i += 1024) {
        uint32_t k = 0;
        for (uint32_t j = 0; j < 4; ++j) k = k << 8 | in[(i + j) % n];
        ka[i] = k;
        ia[i] = i;
    }
    __syncthreads();
    uint32_t passes = 4;
    uint64_t k = 4;
    for (uint32_t round = 0; round < 22; ++round) { // (k reaches n within 20 doublings: the bound holds whatever the data)
        for (uint32_t p = 0; p < passes; ++p) {
            radix_pass(ka, ia, kb, ib, n, p * 8, hist, tmp);
            uint64_t* tk = ka; ka = kb; kb = tk;
            uint32_t* ti = ia; ia = ib; ib = ti;
        }
        // dense ranks from the key-changed flags
        uint32_t carry = 0;
        for (uint32_t base = 0; base < n; base += 1024) {
            const uint32_t j = base + tid;
            const bool valid = j < n;
            const bool flag = valid && (j == 0 || ka[j] != ka[j - 1]);
            uint32_t tot;
            const uint32_t r = carry + block_scan<false>(flag ? 1u : 0u, tmp, &tot);
            carry += tot;
            if (valid) {
                const uint32_t i = ia[j];
                if (i < n) rank[i] = r - 1;
            }
        }
        __syncthreads();
        if (carry == n || k >= n) break; // (carry is the same in every lane)
        for (uint32_t j = tid; j < n; j += 1024) {
            const uint32_t i = ia[j];
            uint64_t i2 = i + k;
            if (i2 >= n) i2 -= n; // (k < n here)
            ka[j] = (uint64_t)rank[i] << rbits | rank[i2];
        }
        __syncthreads();
        passes = (2 * rbits + 7) / 8;
        k *= 2;
    }
    for (uint32_t j = tid; j < n; j += 1024) {
        const uint32_t i = ia[j];
        out[j] = in[i ? i - 1 : n - 1];
        if (i == 0) d_op[(uint64_t)b * op_stride] = j;
    }
}

__global__ void __launch_bounds__(64) bz_enc_mtf_kernel(BzEncScratch s)
{
    __shared__ BzEncMap m;
    const uint32_t b = blockIdx.x, lane = threadIdx.x;
    const uint32_t n = s.res[b].rle_n, room = s.cap + 64;
    const uint8_t* last = s.last + (uint64_t)b * room;
    uint16_t* syms = s.syms + (uint64_t)b * room;
    for (uint32_t c = lane; c < 256; c += 64) m.used[c] = 0;
    __syncthreads();
    for (uint32_t i = lane; i < n; i += 64) m.used[last[i]] = 1;
    __syncthreads();
    if (lane == 0) bzenc_map_finish(m);
    __syncthreads();
    for (uint32_t k = lane; k < sizeof(BzEncMap) / 4; k += 64) ((uint32_t*)&s.maps[b])[k] = ((const uint32_t*)&m)[k];
    // the list, four entries a lane: entry 4 * lane + j in byte j
    uint32_t list = (lane * 4) | (lane * 4 + 1) << 8 | (lane * 4 + 2) << 16 | (lane * 4 + 3) << 24;
    const auto put = [=](uint32_t at, uint16_t v) { // the wave counts, lane 0 stores
        if (lane == 0 && at < room) syms[at] = v;
    };
    uint32_t front = 0, run = 0, w = 0, head = 0x03020100u; // head: lane 0's word, a scalar copy
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t i = base + lane;
        const uint32_t mine = i < n ? m.seq[last[i]] : 0u;
        const uint32_t cnt = min(64u, n - base);
        for (uint32_t t = 0; t < cnt; ++t) {
            const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)t);
            if (v == front) {
                ++run;
                continue;
            }
            if (run) {
                w = bzenc_put_run_to(put, w, run);
                run = 0;
            }
            uint32_t p;
            const uint32_t x0 = head ^ (v * 0x01010101u);
            const uint32_t z0 = (x0 - 0x01010101u) & ~x0 & 0x80808080u; // its lowest set bit marks the lowest zero byte of x0
            if (z0) { // among the first four entries (most symbols behind a BWT are): lane 0's word alone, in scalar registers
                p = (uint32_t)(__ffs((int)z0) - 1) >> 3; // 1..3 (0 is the front)
                const uint32_t mask = p == 3 ? 0xffffffffu : (1u << (8 * (p + 1))) - 1u;
                head = ((head << 8 | v) & mask) | (head & ~mask);
                if (lane == 0) list = head;
            } else {
                const uint32_t x = list ^ (v * 0x01010101u);
                const uint32_t kk = !(x & 0xffu) ? 0u : !(x & 0xff00u) ? 1u : !(x & 0xff0000u) ? 2u : !(x & 0xff000000u) ? 3u : 4u;
                const uint64_t hit = __ballot(kk < 4);
                const uint32_t lp = hit ? (uint32_t)(__ffsll((long long)hit) - 1) : 0u; // (the list holds every value once)
                const uint32_t kq = (uint32_t)__builtin_amdgcn_readlane((int)kk, (int)lp) & 3u;
                // every lane takes its left neighbour's word (DPP wave_shr:1); lane 0, which has none, keeps v << 24
                const uint32_t up = (uint32_t)__builtin_amdgcn_update_dpp((int)(v << 24), (int)list, 0x138, 0xf, 0xf, false);
                const uint32_t shifted = list << 8 | up >> 24;
                if (lane < lp) {
                    list = shifted;
                } else if (lane == lp) {
                    const uint32_t mask = kq == 3 ? 0xffffffffu : (1u << (8 * (kq + 1))) - 1u;
                    list = (shifted & mask) | (list & ~mask);
                }
                head = (uint32_t)__builtin_amdgcn_readlane((int)list, 0);
                p = lp * 4 + kq;
            }
            front = v;
            put(w++, (uint16_t)(p + 1));
        }
    }
    if (run) w = bzenc_put_run_to(put, w, run);
    if (lane == 0) {
        if (w < room) syms[w] = (uint16_t)(m.nused + 1);
        else atomicOr(&s.res[b].over, 1u);
        s.res[b].nmtf = w < room ? w + 1 : 0u;
    }
}

__global__ void __launch_bounds__(1024) bz_enc_code_kernel(const BzEncJob* __restrict__ jobs, BzEncScratch s)
{
    __shared__ BzEncHuff h;
    __shared__ BzEncHuffScratch sc[6];
    __shared__ BzEncMap m;
    __shared__ uint32_t tmp[16];
    __shared__ uint32_t head_bits;
    const uint32_t b = blockIdx.x, tid = threadIdx.x, room = s.cap + 64;
    const uint32_t nmtf = s.res[b].nmtf;
    if (nmtf == 0 || nmtf > room) { // (a stage before this one met its buffer's end)
        if (tid == 0) s.res[b].bits = 0;
        return;
    }
    const uint16_t* syms = s.syms + (uint64_t)b * room;
    uint8_t* sel = s.sel + (uint64_t)b * kBzEncSelStride;
    uint32_t* slot = s.slots + (uint64_t)b * s.slot_words;
    for (uint32_t k = tid; k < sizeof(BzEncMap) / 4; k += 1024) ((uint32_t*)&m)[k] = ((const uint32_t*)&s.maps[b])[k];
    for (uint32_t k = tid; k < kBzEncAlphaMax; k += 1024) h.freq[k] = 0;
    __syncthreads();
    const uint32_t alpha = min(m.nused, 256u) + 2, nt = bzenc_ntables(nmtf), ng = bzenc_groups(nmtf);
    if (ng > kBzEncSelStride) {
        if (tid == 0) { s.res[b].bits = 0; atomicOr(&s.res[b].over, 1u); }
        return;
    }
    for (uint32_t i = tid; i < nmtf; i += 1024) atomicAdd(&h.freq[min((uint32_t)syms[i], alpha - 1)], 1u);
    __syncthreads();
    if (tid == 0) bzenc_initial_lens(h, alpha, nt, nmtf);
    __syncthreads();
    for (uint32_t r = 0; r < kBzEncRounds; ++r) {
        for (uint32_t k = tid; k < 6 * kBzEncAlphaMax; k += 1024) (&h.rfreq[0][0])[k] = 0;
        __syncthreads();
        for (uint32_t g = tid; g < ng; g += 1024) {
            const uint32_t g0 = g * kBzEncGroup, cnt = min(kBzEncGroup, nmtf - g0);
            const uint32_t t = bzenc_pick_table(h, nt, syms + g0, cnt);
            sel[g] = (uint8_t)t;
            for (uint32_t i = 0; i < cnt; ++i) atomicAdd(&h.rfreq[t][syms[g0 + i]], 1u);
        }
        __syncthreads();
        if ((tid & 63) == 0 && (tid >> 6) < nt) bzenc_code_lengths(h.rfreq[tid >> 6], alpha, kBzEncMaxBits, h.len[tid >> 6], sc[tid >> 6]); // a wave a table
        __syncthreads();
    }
    if ((tid & 63) == 0 && (tid >> 6) < nt) bzenc_assign_codes(h.len[tid >> 6], alpha, h.code[tid >> 6]);
    __syncthreads();
    // each lane's run of consecutive groups: their bit lengths, then where the run starts
    const uint32_t per = (ng + 1023) / 1024;
    const uint32_t ga = min(ng, tid * per), ge = min(ng, (tid + 1) * per);
    uint32_t mine = 0;
    for (uint32_t g = ga; g < ge; ++g) {
        const uint32_t g0 = g * kBzEncGroup, cnt = min(kBzEncGroup, nmtf - g0);
        mine += bzenc_group_bits(h, sel[g], syms + g0, cnt);
    }
    uint32_t total;
    const uint32_t at = block_scan<false>(mine, tmp, &total) - mine;
    if (tid == 0) {
        BzW w;
        bzw_start(w, slot, s.slot_words, 0);
        bzenc_write_head(w, jobs[b].crc, s.res[b].orig_ptr, m, h, nt, sel, ng);
        head_bits = (uint32_t)bzw_pos(w);
        bzw_flush(w);
        if (w.over) atomicOr(&s.res[b].over, 1u);
    }
    __syncthreads();
    if (ga < ge) {
        BzW w;
        bzw_start(w, slot, s.slot_words, (uint64_t)head_bits + at);
        for (uint32_t g = ga; g < ge; ++g) {
            const uint32_t g0 = g * kBzEncGroup, cnt = min(kBzEncGroup, nmtf - g0);
            bzenc_write_group(w, h, sel[g], syms + g0, cnt);
        }
        bzw_flush(w);
        if (w.over) atomicOr(&s.res[b].over, 1u);
    }
    if (tid == 0) s.res[b].bits = head_bits + total;
}

__global__ void __launch_bounds__(256) bz_enc_concat_kernel(BzEncScratch s, const uint64_t* __restrict__ dst, uint32_t* out, uint64_t out_words,
                                                            uint32_t carry)
{
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    if (b == 0 && blockIdx.y == 0 && tid == 0 && (carry & 0xffu) && out_words) atomicOr(&out[0], carry & 0xffu); // byte 0 of the stream
    const uint64_t B = s.res[b].bits, D = dst[b];
    if (B == 0) return;
    const uint32_t* src = s.slots + (uint64_t)b * s.slot_words;
    const uint64_t w0 = D >> 5, w1 = (D + B - 1) >> 5, nsw = min((B + 31) / 32, (uint64_t)s.slot_words);
    const uint32_t sh = (uint32_t)(D & 31);
    for (uint64_t wj = w0 + (uint64_t)blockIdx.y * 256 + tid; wj <= w1; wj += (uint64_t)gridDim.y * 256) {
        const uint64_t k = wj - w0; // destination word wj holds source bits [32 k - sh, 32 k - sh + 32)
        const uint32_t hi = (k >= 1 && k - 1 < nsw) ? bzenc_bswap(src[k - 1]) : 0u;
        const uint32_t lo = k < nsw ? bzenc_bswap(src[k]) : 0u;
        const uint32_t v = bzenc_bswap(__builtin_amdgcn_alignbit(hi, lo, sh));
        if (wj >= out_words) continue;
        if (wj == w0 || wj == w1) { // shared with the neighbours
            if (v) atomicOr(&out[wj], v);
        } else {
            out[wj] = v;
        }
    }
}

} // namespace

hipError_t launch_bzenc_blocks(const uint8_t* d_in, const BzEncJob* d_jobs, const BzEncScratch& s, uint32_t nblk, hipStream_t st, hipEvent_t* ev)
{
    if (nblk == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(s.res, 0, (size_t)nblk * sizeof(BzEncRes), st);
    if (!e) e = hipMemsetAsync(s.slots, 0, (size_t)nblk * s.slot_words * 4, st);
    if (!e && ev) e = hipEventRecord(ev[0], st);
    if (e) return e;
    bz_enc_rle1_kernel<<<nblk, 1024, 0, st>>>(d_in, d_jobs, s);
    if (ev) e = hipEventRecord(ev[1], st);
    if (e) return e;
    bz_enc_bwt_kernel<<<nblk, 1024, 0, st>>>(s.rle, s.bwt_jobs, s.last, &s.res[0].orig_ptr, (uint32_t)(sizeof(BzEncRes) / 4), s);
    if (ev) e = hipEventRecord(ev[2], st);
    if (e) return e;
    bz_enc_mtf_kernel<<<nblk, 64, 0, st>>>(s);
    if (ev) e = hipEventRecord(ev[3], st);
    if (e) return e;
    bz_enc_code_kernel<<<nblk, 1024, 0, st>>>(d_jobs, s);
    if (ev) e = hipEventRecord(ev[4], st);
    if (e) return e;
    return hipGetLastError();
}

hipError_t launch_bzenc_from_last(const BzEncJob* d_jobs, const BzEncScratch& s, uint32_t nblk, hipStream_t st)
{
    if (nblk == 0) return hipSuccess;
    const hipError_t e = hipMemsetAsync(s.slots, 0, (size_t)nblk * s.slot_words * 4, st);
    if (e) return e;
    bz_enc_mtf_kernel<<<nblk, 64, 0, st>>>(s);
    bz_enc_code_kernel<<<nblk, 1024, 0, st>>>(d_jobs, s);
    return hipGetLastError();
}

hipError_t launch_bzenc_bwt(const uint8_t* d_in, const BzBwtJob* d_jobs, uint8_t* d_out, uint32_t* d_op, const BzEncScratch& s, uint32_t nblk,
                            hipStream_t st)
{
    if (nblk == 0) return hipSuccess;
    bz_enc_bwt_kernel<<<nblk, 1024, 0, st>>>(d_in, d_jobs, d_out, d_op, 1u, s);
    return hipGetLastError();
}

hipError_t launch_bzenc_concat(const BzEncScratch& s, const uint64_t* d_dst, uint32_t nblk, uint32_t* d_out, uint64_t out_words, uint32_t carry,
                               hipStream_t st)
{
    if (nblk == 0 || out_words == 0) return hipSuccess;
    const hipError_t e = hipMemsetAsync(d_out, 0, (size_t)out_words * 4, st);
    if (e) return e;
    bz_enc_concat_kernel<<<dim3(nblk, 8), 256, 0, st>>>(s, d_dst, d_out, out_words, carry);
    return hipGetLastError();
}

} // namespace snaphash
