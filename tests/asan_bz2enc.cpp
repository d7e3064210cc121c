// asan_bz2enc.cpp -- the .bz2 writer's host model (snappy_amd/csrc/bzip2_enc_core.h) and bzip2_core.h's decoder over what
// it wrote, as a program of its own for -fsanitize=address,undefined (tests/test_bz2enc_host.py builds and runs it; nothing
// here is loaded into python).  Arguments: a count of random inputs, a seed, then pairs of (input file, level).  Each
// input is read into a heap buffer of exactly its size, encoded, decoded block by block with bz_block_symbols / bz_ibwt /
// bz_rle1 and compared: "ok" an input, exit 0 when all are.  "-e" / "-l" in place of an input file begins an edge input of
// tests/bz2enc_cases.py for the stage model (bz2enc_stage_model.h): -e DATA RANGES LEVEL CAP CARRY CARRY_BITS with RANGES a
// text file of "offset length" lines, -l likewise for the from_last mode with DATA the last columns one after the other
// and RANGES "offset length origPtr crc" lines.  Every array is a heap buffer of exactly its size; each slot is read back
// with bz_block_symbols and compared with the block's last column, origPtr and CRC.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bz2enc_stage_model.h"

using namespace snaphash;

static std::vector<uint8_t> read_exact(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) { printf("open\n"); exit(2); }
    std::vector<uint8_t> big(8u << 20);
    const size_t n = fread(big.data(), 1, big.size(), f);
    fclose(f);
    return std::vector<uint8_t>(big.begin(), big.begin() + (long)n); // (no byte behind the input may be read)
}

// one edge input through the stage model; from_last: rows of (offset, length, origPtr, crc), else (offset, length)
static bool stages_round(const std::vector<uint8_t>& data, const std::vector<uint64_t>& rows, bool from_last, uint32_t level, uint32_t cap,
                         uint32_t carry, uint32_t carry_bits)
{
    const uint32_t per = from_last ? 4 : 2, nblk = (uint32_t)(rows.size() / per);
    if (cap == 0) cap = (bzenc_rle_cap(level) + 63) & ~63u;
    const size_t room = cap + 64, sw = bzenc_slot_words(cap);
    std::vector<uint8_t> rle(nblk * room, kBeFill), last(nblk * room, kBeFill), maps(nblk * sizeof(BzEncMap), kBeFill), sel((size_t)nblk * kBeSelStride, kBeFill),
        over(nblk, 0);
    std::vector<uint16_t> syms(nblk * room, (uint16_t)(kBeFill * 0x101));
    std::vector<uint32_t> slots(nblk * sw, 0u), res((size_t)nblk * kBeResWords, 0u), out(nblk * sw + 2, 0u);
    std::vector<uint64_t> dst(nblk, 0), offs(nblk), lens(nblk);
    std::vector<uint32_t> rn(nblk), op(nblk), crc(nblk);
    for (uint32_t k = 0; k < nblk; ++k) {
        offs[k] = rows[(size_t)k * per];
        lens[k] = rows[(size_t)k * per + 1];
        if (offs[k] + lens[k] > data.size() || lens[k] == 0) return false;
        if (from_last) {
            if (lens[k] > cap) return false;
            rn[k] = (uint32_t)lens[k]; op[k] = (uint32_t)rows[(size_t)k * 4 + 2]; crc[k] = (uint32_t)rows[(size_t)k * 4 + 3];
            memcpy(last.data() + k * room, data.data() + offs[k], lens[k]);
        } else if (lens[k] > bzenc_piece(level)) {
            return false;
        }
    }
    const BeArrays a = {rle.data(), last.data(), syms.data(), maps.data(), sel.data(), slots.data(), res.data(), dst.data(), out.data(), out.size(), over.data()};
    const int64_t total = from_last ? be_stages_from_last_host(rn.data(), op.data(), crc.data(), nblk, cap, carry, carry_bits, a)
                                    : be_stages_host(data.data(), offs.data(), lens.data(), nblk, cap, carry, carry_bits, a);
    uint64_t at = carry_bits;
    bool any_over = false;
    std::vector<uint8_t> back(room);
    for (uint32_t k = 0; k < nblk; ++k) {
        if (over[k]) { any_over = true; continue; }
        const uint32_t* r = res.data() + (size_t)k * kBeResWords;
        uint32_t n2, op2, crc2;
        uint64_t end;
        std::vector<uint32_t> slot(slots.begin() + (long)(k * sw), slots.begin() + (long)((k + 1) * sw)); // (exactly its size)
        if (be_read_slot_host(slot.data(), (uint32_t)sw, back.data(), (uint32_t)room, &n2, &op2, &crc2, &end) != kBzOk) return false;
        if (n2 != r[0] || op2 != r[1] || end != r[3] || memcmp(back.data(), last.data() + k * room, n2)) return false;
        if (from_last && (crc2 != crc[k] || op2 != op[k])) return false;
        at += r[3];
    }
    return any_over ? total == -1 : total == (int64_t)at;
}

static std::vector<uint64_t> read_rows(const char* path)
{
    std::vector<uint64_t> rows;
    FILE* f = fopen(path, "r");
    if (!f) { printf("open\n"); exit(2); }
    unsigned long long v;
    while (fscanf(f, "%llu", &v) == 1) rows.push_back(v);
    fclose(f);
    return rows;
}

static bool round_trip(const std::vector<uint8_t>& exact, uint32_t level)
{
    std::vector<BzEncBlockInfo> infos;
    const std::vector<uint8_t> z0 = bzenc_stream_host(exact.data(), exact.size(), level, &infos);
    std::vector<uint8_t> z(z0); // (exactly its size)
    if (z.size() < 14 || z[0] != 'B' || z[1] != 'Z' || z[2] != 'h' || z[3] != '0' + level) return false;
    const uint32_t P = bzenc_piece(level);
    if (infos.size() != (exact.size() + P - 1) / P) return false;
    std::vector<uint8_t> back, bwt(kBzMaxBlock), plain(kBzMaxBlock);
    std::vector<uint32_t> tt(kBzMaxBlock);
    std::vector<BzTables> t(1);
    uint32_t crc_tab[256];
    bz_crc_table(crc_tab);
    uint64_t bit = 32;
    uint32_t fold = 0;
    for (size_t k = 0; k < infos.size(); ++k) {
        uint32_t counts[256];
        const BzBlockRes r = bz_block_symbols(z.data(), z.size(), bit, bwt.data(), kBzMaxBlock, counts, t[0]);
        if (r.status != kBzOk || r.n != infos[k].rle_n || r.orig_ptr != infos[k].orig_ptr || r.end_bit - bit != infos[k].bits) return false;
        bz_ibwt(bwt.data(), r.n, counts, r.orig_ptr, tt.data(), plain.data());
        BzRle1 st;
        const uint64_t at = back.size();
        const uint64_t len = bz_rle1(st, plain.data(), r.n, nullptr, 0);
        back.resize(at + len);
        BzRle1 st2;
        if (bz_rle1(st2, plain.data(), r.n, back.data() + at, len) != len) return false;
        if (~bz_crc_update(crc_tab, ~0u, back.data() + at, len) != r.crc) return false;
        fold = bz_crc_combine(fold, r.crc);
        bit = r.end_bit;
    }
    if (bz_bits48(z.data(), z.size(), bit) != kBzEosMagic) return false;
    BzBits b;
    bb_start(b, z.data(), z.size(), bit + 48);
    if (bb_take(b, 32) != fold) return false;
    return back == exact && (bit + 80 + 7) / 8 == z.size();
}

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const long nrandom = strtol(argv[1], nullptr, 10);
    uint64_t seed = strtoull(argv[2], nullptr, 10) * 2654435761u + 1;
    auto next = [&seed]() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return seed; };
    int bad = 0;
    for (int i = 3; i + 1 < argc; i += 2) {
        if (argv[i][0] == '-' && i + 6 < argc) { // an edge input of the stage model
            const bool from_last = argv[i][1] == 'l';
            const std::vector<uint8_t> data = read_exact(argv[i + 1]);
            const std::vector<uint64_t> rows = read_rows(argv[i + 2]);
            const bool ok = rows.size() % (from_last ? 4 : 2) == 0 &&
                            stages_round(data, rows, from_last, (uint32_t)strtoul(argv[i + 3], nullptr, 10), (uint32_t)strtoul(argv[i + 4], nullptr, 10),
                                         (uint32_t)strtoul(argv[i + 5], nullptr, 10), (uint32_t)strtoul(argv[i + 6], nullptr, 10));
            printf(ok ? "ok\n" : "FAILED\n");
            bad += !ok;
            i += 5;
            continue;
        }
        const std::vector<uint8_t> exact = read_exact(argv[i]);
        const bool ok = round_trip(exact, (uint32_t)strtoul(argv[i + 1], nullptr, 10));
        printf(ok ? "ok\n" : "FAILED\n");
        bad += !ok;
    }
    // random inputs of random length and level: alphabets of 1 to 256 values, with and without runs
    long good = 0;
    for (long k = 0; k < nrandom; ++k) {
        const uint64_t shape = next();
        size_t n = (size_t)(next() % ((shape & 15) == 0 ? 200u * 1024 + 1 : 3000));
        const uint32_t level = 1 + (uint32_t)(next() % 9), alpha = 1 + (uint32_t)(next() % 256), runs = (uint32_t)(shape >> 8 & 3);
        std::vector<uint8_t> exact(n);
        for (size_t i = 0; i < n;) {
            const uint8_t v = (uint8_t)(next() % alpha);
            size_t len = runs == 0 ? 1 : 1 + (size_t)(next() % (runs == 1 ? 6 : 600));
            for (; len && i < n; --len) exact[i++] = v;
        }
        if (round_trip(exact, level)) ++good;
        else { printf("FAILED random %ld (n %zu level %u alpha %u runs %u)\n", k, n, level, alpha, runs); ++bad; }
    }
    printf("random %ld\n", good);
    return bad ? 1 : 0;
}
