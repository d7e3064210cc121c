// inflate_core.h -- the RFC 1951 decoder of the install side, shared by the GPU inflate kernel
// (inflate_kernels.hip), the library's host decoder (inflate_host.cpp) and a host harness in tests/, the way
// deflate_core.h serves the compressor and its CPU model.
//
// One routine, inflate_run, decodes from a start bit either to the end of the final block or -- stop_at_flush -- to the
// end of the next non-final stored block: the empty one of zlib's Z_SYNC_FLUSH / Z_FULL_FLUSH (the bytes 00 00 FF FF
// after the header bits; the producer writes one after every 64 KiB chunk it compresses, deflate_kernels.hip) or a
// stored chunk (the producer's chunks that do not shrink).  Either ends on a byte boundary, where the next block starts.
// Such a stretch is a *segment*: it can be decoded without the bytes before it, except for back-references that reach
// in front of its start.  With `holes` set (T = uint16_t) such a reference is not an error: the output symbol becomes
// kInfHole + w, "the byte w bytes before the first byte in front of out[-hist]", to be filled in once the segment
// before it is known.  Without it
// (T = uint8_t) the `hist` bytes in front of `out` are the window and a reference beyond them is an error.
//
// Every path is bounded: input past the end reads as zeros and ends the run as kInfTruncated, output past `cap` ends it
// as kInfOverflow, anything RFC 1951 forbids as kInfBad -- a false segment start (00 00 FF FF inside stored data) or a
// corrupt stream never reads or writes out of bounds.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define IF_HD __host__ __device__ inline
#else
#define IF_HD inline
#endif

namespace snaphash {

constexpr uint32_t kInfHole = 256;       // output symbol >= kInfHole: a hole (T = uint16_t only)
constexpr uint32_t kInfWindow = 32768;   // farthest back-reference RFC 1951 allows
constexpr uint32_t kInfFastBits = 9;     // first-level lookup of a Huffman code (longer codes: canonical walk)

enum : int32_t {
    kInfFinal = 0,     // decoded through the end of the final block
    kInfFlush = 1,     // stopped after a non-final stored block (stop_at_flush); end_bit is byte aligned
    kInfTruncated = 2, // the input ended first
    kInfOverflow = 3,  // the output would pass cap
    kInfBad = 4,       // not a valid DEFLATE stream (or, without holes, a reference in front of the window)
    kInfBlock = 5,     // block mode: stopped at a block end (any bit alignment); end_bit is the next block's first bit
};

// Block mode (block_min != kInfNoBlockStop): the run stops at the first block end at or after block_min output symbols
// where the next block can start a segment -- a dynamic-Huffman header follows (the block scan finds it), or the block
// that ended was stored (a byte-aligned end, a stored-block candidate).  A fixed or stored block after such an end is
// decoded on into, so that it does not break the chain.  When the output passes cap or the input ends, a run that has
// passed such an end reports the last one instead: status kInfBlock, `cut` = the status it was cut from.
constexpr uint64_t kInfNoBlockStop = ~0ull;

struct InflateRun {
    uint64_t end_bit = 0;  // first bit after what was decoded
    uint64_t out_len = 0;  // output symbols written
    uint32_t hole_end = 0; // 1 + the last output position that holds a hole (0: none)
    int32_t status = kInfBad;
    int32_t cut = 0;       // block mode: kInfOverflow / kInfTruncated if the run was rolled back to its last block end
};

// A canonical Huffman code: counts per length, symbols in code order, and a first-level table of
// (length << 9 | symbol) for the codes of up to kInfFastBits bits (0: a longer code starts with these bits).
struct InflateCode {
    uint16_t count[16];
    uint16_t sym[288];
    uint16_t fast[1u << kInfFastBits];
};

struct InflateTables {
    InflateCode lit, dist;
    uint16_t lens[320]; // code lengths of a dynamic block (286 + 30 at most, and the 19 of the code-length code)
};

struct InfBits {
    const uint8_t* in;
    uint64_t n;   // input bytes
    uint64_t pos; // next byte to load (may pass n: the bytes past the end read as zeros)
    uint64_t buf;
    uint32_t cnt; // bits in buf
};

IF_HD void ib_fill(InfBits& b)
{
    while (b.cnt <= 56) {
        const uint64_t v = b.pos < b.n ? b.in[b.pos] : 0;
        b.buf |= v << b.cnt;
        ++b.pos;
        b.cnt += 8;
    }
}
IF_HD uint64_t ib_consumed(const InfBits& b) { return b.pos * 8 - b.cnt; }
IF_HD bool ib_over(const InfBits& b) { return b.pos > b.n && ib_consumed(b) > b.n * 8; }
IF_HD uint32_t ib_take(InfBits& b, uint32_t k) // k <= 32, after ib_fill left enough bits
{
    const uint32_t v = (uint32_t)(b.buf & ((1ull << k) - 1));
    b.buf >>= k;
    b.cnt -= k;
    return v;
}

// Builds the code from n lengths.  Returns false for an over-subscribed code and for an incomplete one unless it is a
// single code of length 1 (zlib's inflate_table rule); a code with no symbols at all is accepted (it is an error to use it).
IF_HD bool inf_build(InflateCode& h, const uint16_t* len, uint32_t n, bool allow_single)
{
    for (uint32_t i = 0; i < 16; ++i) h.count[i] = 0;
    for (uint32_t i = 0; i < n; ++i) h.count[len[i]]++;
    for (uint32_t i = 0; i < (1u << kInfFastBits); ++i) h.fast[i] = 0;
    if (h.count[0] == n) return true;
    int32_t left = 1;
    uint32_t maxlen = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        left <<= 1;
        left -= h.count[l];
        if (left < 0) return false;
        if (h.count[l]) maxlen = l;
    }
    if (left > 0 && !(allow_single && maxlen == 1)) return false;
    uint16_t offs[16];
    offs[1] = 0;
    for (uint32_t l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + h.count[l]);
    uint32_t next[16]; // first code of each length (RFC 1951 sec. 3.2.2)
    next[1] = 0;
    for (uint32_t l = 2; l < 16; ++l) next[l] = (next[l - 1] + h.count[l - 1]) << 1;
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = len[s];
        if (l == 0) continue;
        h.sym[offs[l]++] = (uint16_t)s;
        const uint32_t c = next[l]++;
        if (l > kInfFastBits) continue;
        uint32_t r = 0; // the code's bits in stream order (Huffman codes go MSB first)
        for (uint32_t k = 0; k < l; ++k) r |= ((c >> k) & 1u) << (l - 1 - k);
        for (uint32_t f = r; f < (1u << kInfFastBits); f += 1u << l) h.fast[f] = (uint16_t)((l << 9) | s);
    }
    return true;
}

// One symbol; -1 for bits that are no code.  Needs 15 bits in the buffer.
IF_HD int32_t inf_decode(InfBits& b, const InflateCode& h)
{
    const uint32_t e = h.fast[b.buf & ((1u << kInfFastBits) - 1)];
    if (e) {
        ib_take(b, e >> 9);
        return (int32_t)(e & 511);
    }
    int32_t code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        code |= (int32_t)ib_take(b, 1);
        const int32_t count = h.count[l];
        if (code - count < first) return h.sym[index + (code - first)];
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

IF_HD void inf_fixed(InflateTables& t)
{
    for (uint32_t i = 0; i < 144; ++i) t.lens[i] = 8;
    for (uint32_t i = 144; i < 256; ++i) t.lens[i] = 9;
    for (uint32_t i = 256; i < 280; ++i) t.lens[i] = 7;
    for (uint32_t i = 280; i < 288; ++i) t.lens[i] = 8;
    inf_build(t.lit, t.lens, 288, false);
    for (uint32_t i = 0; i < 32; ++i) t.lens[i] = 5; // (30 and 31 complete the code and are refused when they occur)
    inf_build(t.dist, t.lens, 32, false);
}

// A dynamic block's header (RFC 1951 sec. 3.2.7) into t.  false: invalid or truncated (the caller tells them apart).
IF_HD bool inf_dynamic(InfBits& b, InflateTables& t)
{
    ib_fill(b);
    const uint32_t nlen = ib_take(b, 5) + 257, ndist = ib_take(b, 5) + 1, ncode = ib_take(b, 4) + 4;
    if (nlen > 286 || ndist > 30) return false;
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint16_t cl[19];
    for (uint32_t i = 0; i < 19; ++i) cl[i] = 0;
    ib_fill(b);
    for (uint32_t i = 0; i < ncode; ++i) cl[order[i]] = (uint16_t)ib_take(b, 3);
    if (!inf_build(t.lit, cl, 19, false)) return false; // (the code-length code borrows the literal table)
    uint32_t i = 0;
    while (i < nlen + ndist) {
        ib_fill(b);
        if (ib_over(b)) return false;
        const int32_t s = inf_decode(b, t.lit);
        if (s < 0) return false;
        if (s < 16) { t.lens[i++] = (uint16_t)s; continue; }
        uint32_t rep, val = 0;
        if (s == 16) {
            if (i == 0) return false;
            val = t.lens[i - 1];
            rep = 3 + ib_take(b, 2);
        } else if (s == 17) {
            rep = 3 + ib_take(b, 3);
        } else {
            rep = 11 + ib_take(b, 7);
        }
        if (i + rep > nlen + ndist) return false;
        while (rep--) t.lens[i++] = (uint16_t)val;
    }
    if (t.lens[256] == 0) return false; // no end-of-block code
    // t.lens is the literal table's input and the distance lengths follow it: build the distance code first
    if (!inf_build(t.dist, t.lens + nlen, ndist, true)) return false;
    return inf_build(t.lit, t.lens, nlen, true);
}

// ---- the block-boundary scan's test (inflate_kernels.hip inflate_block_scan_kernel) --------------------------------
// inf_dynamic_ok(in, n, bit): does a block with BTYPE = 2 start at `bit` whose header inf_dynamic accepts, read from
// in[0..n) with the bytes past n as zeros, and does that header end within the n bytes?  The same answer as inf_dynamic,
// without its tables: the code-length ("precode") code is kept as 19 packed 3-bit lengths and decoded by its canonical
// order; the literal/length and distance codes only need counts, so a Kraft sum (in units of 2^-15), the largest length
// and the number of used lengths stand in for inf_build.  Registers only.
// Bits read from `bit` at most: 3 + 14 + 19 * 3 = 74 for the block and precode headers, then at most 286 + 30 = 316
// code lengths at most 7 bits each (a repeat code spends at most 14 bits on 3 or more lengths), so 74 + 316 * 7 = 2286.
constexpr uint32_t kInfHeaderMaxBits = 2286;

// 64 bits of in[0..n) from bit `at` on (zeros past n); the first 57 are always whole
IF_HD uint64_t inf_peek64(const uint8_t* in, uint64_t n, uint64_t at)
{
    const uint64_t p = at >> 3;
    uint64_t v = 0;
    for (uint32_t k = 0; k < 8; ++k) v |= (uint64_t)(p + k < n ? in[p + k] : 0) << (8 * k);
    return v >> (at & 7);
}

struct InfDynHead {
    uint64_t cl;   // the 19 precode lengths, 3 bits each, by symbol
    uint64_t cnt;  // precode lengths per length 1..7, 8 bits each (byte l)
    uint32_t nlen, ndist;
    uint64_t next; // the first bit after the precode lengths
};

// The cheap half: BTYPE, HLIT, HDIST, HCLEN and a complete precode (inf_build of 19 lengths, no single code allowed; an
// all-zero precode builds, then fails at the first length, so it is refused here).
IF_HD bool inf_dynamic_head(const uint8_t* in, uint64_t n, uint64_t bit, InfDynHead& h)
{
    const uint64_t w = inf_peek64(in, n, bit);
    if (((w >> 1) & 3) != 2) return false;
    h.nlen = (uint32_t)((w >> 3) & 31) + 257;
    h.ndist = (uint32_t)((w >> 8) & 31) + 1;
    const uint32_t ncode = (uint32_t)((w >> 13) & 15) + 4;
    if (h.nlen > 286 || h.ndist > 30) return false;
    const uint64_t v = inf_peek64(in, n, bit + 17); // the precode lengths in stream order: 57 bits at most
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    h.cl = 0;
    h.cnt = 0;
    uint32_t kraft = 0; // in units of 2^-7
    for (uint32_t i = 0; i < ncode; ++i) {
        const uint32_t l = (uint32_t)(v >> (3 * i)) & 7;
        h.cl |= (uint64_t)l << (3 * order[i]);
        if (l) {
            kraft += 128u >> l;
            h.cnt += 1ull << (8 * l);
        }
    }
    h.next = bit + 17 + 3 * ncode;
    return kraft == 128;
}

// The code-length walk after inf_dynamic_head: every rule of inf_dynamic and inf_build.
IF_HD bool inf_dynamic_lengths(const uint8_t* in, uint64_t n, const InfDynHead& h)
{
    const uint32_t total = h.nlen + h.ndist;
    uint64_t at = h.next;
    uint32_t i = 0, prev = 0, at256 = 0;
    uint32_t lk = 0, dk = 0, lmax = 0, dmax = 0, dused = 0; // Kraft sums in units of 2^-15, largest lengths, used codes
    while (i < total) {
        if (at > n * 8) return false; // (inf_dynamic's ib_over before each symbol)
        uint64_t w = inf_peek64(in, n, at);
        // canonical decode of the complete precode (RFC 1951 sec. 3.2.2): at most 7 bits
        uint32_t code = 0, first = 0, s = 19, l = 1;
        for (; l <= 7; ++l) {
            code |= (uint32_t)(w >> (l - 1)) & 1;
            const uint32_t c = (uint32_t)(h.cnt >> (8 * l)) & 255;
            if (code - first < c) { // the (code - first)-th symbol of length l, in symbol order
                uint32_t k = code - first;
                for (uint32_t q = 0; q < 19; ++q)
                    if (((h.cl >> (3 * q)) & 7) == l) {
                        if (k == 0) { s = q; break; }
                        --k;
                    }
                break;
            }
            first = (first + c) << 1;
            code <<= 1;
        }
        if (s == 19) return false; // (cannot happen: the precode is complete)
        w >>= l;
        at += l;
        uint32_t rep, val;
        if (s < 16) {
            rep = 1;
            val = s;
        } else if (s == 16) {
            if (i == 0) return false;
            rep = 3 + ((uint32_t)w & 3);
            val = prev;
            at += 2;
        } else if (s == 17) {
            rep = 3 + ((uint32_t)w & 7);
            val = 0;
            at += 3;
        } else {
            rep = 11 + ((uint32_t)w & 127);
            val = 0;
            at += 7;
        }
        if (i + rep > total) return false;
        if (val) { // the lengths i .. i+rep-1: literal/length code below nlen, distance code from there
            const uint32_t nl = i < h.nlen ? (i + rep < h.nlen ? rep : h.nlen - i) : 0;
            lk += nl << (15 - val);
            dk += (rep - nl) << (15 - val);
            if (nl) lmax = lmax > val ? lmax : val;
            if (rep - nl) { dmax = dmax > val ? dmax : val; dused += rep - nl; }
            if (lk > 32768 || dk > 32768) return false; // over-subscribed: only grows
            if (i <= 256 && 256 < i + rep) at256 = 1;
        }
        prev = val;
        i += rep;
    }
    if (!at256) return false;                                       // no end-of-block code
    if (at > n * 8) return false;                                   // the header runs past the piece
    if (dused && dk < 32768 && dmax != 1) return false;             // incomplete distance code, not a single code
    return lk == 32768 || lmax == 1;                                // (lens[256] != 0: the literal code is not empty)
}

IF_HD bool inf_dynamic_ok(const uint8_t* in, uint64_t n, uint64_t bit)
{
    InfDynHead h;
    return inf_dynamic_head(in, n, bit, h) && inf_dynamic_lengths(in, n, h);
}

// Decodes in[0..n) from start_bit into out[0..cap).  T = uint8_t: out[-hist..-1] is the window; T = uint16_t with holes:
// a reference in front of out[0] becomes a hole symbol.  Stops as described at the top of the file, or in block mode
// (block_min, see kInfNoBlockStop).
template <typename T>
IF_HD InflateRun inflate_run(const uint8_t* in, uint64_t n, uint64_t start_bit, T* out, uint64_t hist, uint64_t cap, bool holes,
                             bool stop_at_flush, InflateTables& t, uint64_t block_min = kInfNoBlockStop)
{
    const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    const uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    const uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
                                6145, 8193, 12289, 16385, 24577};
    const uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    InflateRun r;
    InfBits b;
    b.in = in;
    b.n = n;
    b.pos = start_bit >> 3;
    b.buf = 0;
    b.cnt = 0;
    ib_fill(b);
    ib_take(b, (uint32_t)(start_bit & 7));
    uint64_t o = 0;
    const uint64_t hist_all = hist; // (holes count from the first byte in front of the history)
    if (hist > kInfWindow) hist = kInfWindow;
#define IF_END(st)                       \
    {                                    \
        r.status = (st);                 \
        r.out_len = o;                   \
        r.end_bit = ib_consumed(b);      \
        return r;                        \
    }
    // block mode: the last block end a segment may stop at (see kInfNoBlockStop), for a run that is cut short
    bool have_end = false;
    uint64_t end_bit = 0, end_out = 0;
#define IF_STOP(st)                                                                              \
    {                                                                                            \
        if (!have_end) IF_END(st);                                                               \
        r.status = kInfBlock;                                                                    \
        r.cut = (st);                                                                            \
        r.out_len = end_out;                                                                     \
        r.end_bit = end_bit;                                                                     \
        if (r.hole_end > end_out) r.hole_end = (uint32_t)end_out;                                \
        return r;                                                                                \
    }
#define IF_BLOCK_END(stored)                                                                     \
    if (block_min != kInfNoBlockStop) {                                                          \
        ib_fill(b);                                                                              \
        if ((stored) || ((b.buf >> 1) & 3) == 2) {                                               \
            if (o >= block_min) IF_END(kInfBlock);                                               \
            have_end = true;                                                                     \
            end_bit = ib_consumed(b);                                                            \
            end_out = o;                                                                         \
        }                                                                                        \
    }
    for (;;) {
        ib_fill(b);
        const uint32_t final = ib_take(b, 1), type = ib_take(b, 2);
        if (ib_over(b)) IF_STOP(kInfTruncated);
        if (type == 0) {
            ib_take(b, b.cnt & 7); // to the byte boundary
            const uint64_t at = ib_consumed(b) >> 3;
            if (at + 4 > n) IF_STOP(kInfTruncated);
            const uint32_t len = in[at] | (uint32_t)in[at + 1] << 8, nlen = in[at + 2] | (uint32_t)in[at + 3] << 8;
            if (len != (~nlen & 0xffffu)) IF_END(kInfBad);
            if (at + 4 + len > n) IF_STOP(kInfTruncated);
            if (o + len > cap) IF_STOP(kInfOverflow);
            for (uint32_t i = 0; i < len; ++i) out[o + i] = (T)in[at + 4 + i];
            o += len;
            b.pos = at + 4 + len;
            b.buf = 0;
            b.cnt = 0;
            ib_fill(b);
            if (final) IF_END(kInfFinal);
            if (stop_at_flush) IF_END(kInfFlush);
            IF_BLOCK_END(true);
            continue;
        }
        if (type == 1) {
            inf_fixed(t);
        } else if (type == 2) {
            if (!inf_dynamic(b, t)) {
                if (ib_over(b)) IF_STOP(kInfTruncated);
                IF_END(kInfBad);
            }
        } else {
            IF_END(kInfBad);
        }
        for (;;) {
            ib_fill(b);
            const int32_t s = inf_decode(b, t.lit);
            if (ib_over(b)) IF_STOP(kInfTruncated);
            if (s < 0) IF_END(kInfBad);
            if (s < 256) {
                if (o >= cap) IF_STOP(kInfOverflow);
                out[o++] = (T)s;
                continue;
            }
            if (s == 256) break;
            if (s > 285) IF_END(kInfBad);
            const uint32_t len = lbase[s - 257] + ib_take(b, lext[s - 257]);
            const int32_t ds = inf_decode(b, t.dist);
            if (ds < 0 || ds > 29) IF_END(kInfBad);
            const uint32_t d = dbase[ds] + ib_take(b, dext[ds]);
            if (ib_over(b)) IF_STOP(kInfTruncated);
            if (o + len > cap) IF_STOP(kInfOverflow);
            // a hole copied from inside the segment is a hole too: what may hold one ends at o + len
            if (holes && (int64_t)o - (int64_t)d < (int64_t)r.hole_end) r.hole_end = (uint32_t)(o + len);
            if (o >= d) {
                T* p = out + o;
                const T* q = p - d;
                uint32_t i = 0;
                if (d >= 16) // sixteen loads in flight before their stores (the GPU's loads are long; the source is behind p)
                    for (; i + 16 <= len; i += 16) {
                        T v[16];
                        for (uint32_t k = 0; k < 16; ++k) v[k] = q[i + k];
                        for (uint32_t k = 0; k < 16; ++k) p[i + k] = v[k];
                    }
                for (; i < len; ++i) p[i] = q[i];
            } else {
                for (uint32_t i = 0; i < len; ++i) {
                    const uint64_t at = o + i;
                    if (at >= d) {
                        out[at] = out[at - d];
                    } else if (d - at <= hist) {
                        out[at] = out[(int64_t)at - (int64_t)d];
                    } else if (holes) {
                        out[at] = (T)(kInfHole + (d - at - hist_all));
                    } else {
                        IF_END(kInfBad);
                    }
                }
            }
            o += len;
        }
        if (final) IF_END(kInfFinal);
        IF_BLOCK_END(false);
    }
#undef IF_BLOCK_END
#undef IF_STOP
#undef IF_END
}

} // namespace snaphash
