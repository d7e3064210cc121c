// Test-only (CPU): the engine's owning buffers (snappy_amd/csrc/devbuf.h) and their groups (engine_bufs.h) against a fake
// allocator that can fail its k-th call.  The library defines devbuf_alloc / devbuf_free with hipMalloc and pinned host
// memory; here they are malloc and free, with every live block recorded.  Not part of the product.
//
// usage: devbuf_host <case>   (buf | groups | review | all); prints "<case> ok" and exits 0, or the first failure and 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>

#include "../snappy_amd/csrc/engine_bufs.h"

using namespace snaphash;

namespace {

struct Block { Mem kind; size_t bytes; int node; };
std::map<void*, Block> g_live;
long g_calls = 0;   // allocations asked for so far
long g_fail_at = -1; // the call (0-based) that fails; -1: none

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

void fail_at(long k) { g_calls = 0; g_fail_at = k; }

uint64_t live_bytes()
{
    uint64_t n = 0;
    for (const auto& b : g_live) n += b.second.bytes;
    return n;
}

// every buffer of a group is empty
struct Empty {
    bool ok = true;
    template <class T, Mem K> void operator()(const Buf<T, K>& b) { ok = ok && b.size() == 0 && b.data() == nullptr; }
};
template <class G> bool empty(G& g)
{
    Empty e;
    g.each(e);
    return e.ok;
}

// every buffer of a group is what the allocator handed out, with the bytes it was asked for
struct Recorded {
    bool ok = true;
    template <class T, Mem K> void operator()(const Buf<T, K>& b)
    {
        if (!b.data()) { ok = ok && b.size() == 0; return; }
        auto it = g_live.find(b.data());
        ok = ok && it != g_live.end() && it->second.kind == K && it->second.bytes == b.bytes();
    }
};
template <class G> bool recorded(G& g)
{
    Recorded r;
    g.each(r);
    return r.ok;
}

void case_buf()
{
    fail_at(-1);
    {
        DevBuf<uint32_t> d;
        CHECK(d.reserve(10) == hipSuccess && d.size() == 10 && d.bytes() == 40 && d.data());
        uint32_t* p = d.data();
        CHECK(d.reserve(10) == hipSuccess && d.reserve(3) == hipSuccess && d.data() == p && g_calls == 1); // large enough: kept
        CHECK(g_live.at(p).kind == Mem::Hbm && g_live.at(p).node == -1);
        fail_at(0);
        CHECK(d.reserve(11) == hipErrorOutOfMemory); // grown: the old one goes first, then the new one fails
        CHECK(d.size() == 0 && d.bytes() == 0 && d.data() == nullptr && g_live.empty());
        fail_at(-1);
        CHECK(d.reserve(11) == hipSuccess && d.size() == 11 && live_bytes() == 44);
        DevBuf<uint32_t> e(std::move(d));
        CHECK(d.data() == nullptr && d.size() == 0 && e.size() == 11 && g_live.size() == 1);
        DevBuf<uint32_t> f;
        CHECK(f.reserve(2) == hipSuccess && g_live.size() == 2);
        f = std::move(e); // f's own block is freed
        CHECK(f.size() == 11 && e.size() == 0 && g_live.size() == 1 && live_bytes() == 44);
        f.reset();
        CHECK(f.size() == 0 && f.data() == nullptr && g_live.empty());

        HostBuf<uint64_t> h;
        CHECK(h.reserve(4, 3) == hipSuccess && h.bytes() == 32);
        CHECK(g_live.at(h.data()).kind == Mem::Pinned && g_live.at(h.data()).node == 3);
        h[3] = 7;
        CHECK(h.data()[3] == 7);
        fail_at(0);
        CHECK(h.reserve(5, 3) == hipErrorOutOfMemory && h.size() == 0 && h.data() == nullptr && g_live.empty());
        fail_at(-1);
        CHECK(h.reserve(5, -1) == hipSuccess && g_live.at(h.data()).node == -1);
    }
    CHECK(g_live.empty()); // the destructors free what is left
    printf("buf ok\n");
}

// Every allocation of ensure() fails in turn, on an empty group and on one sized for a smaller job: the group ends empty
// each time, and nothing is left allocated.  Then it succeeds, and every buffer is what the allocator handed out.
template <class G, class Small, class Big> void every_failure(const char* what, Small small, Big big)
{
    fail_at(-1);
    long n_alloc;
    {
        G g;
        CHECK(big(g) == hipSuccess && recorded(g) && !empty(g));
        n_alloc = g_calls;
    }
    CHECK(n_alloc > 0 && g_live.empty());
    for (long k = 0; k < n_alloc; ++k) {
        G g;
        fail_at(k);
        CHECK(big(g) == hipErrorOutOfMemory && empty(g) && g_live.empty());
        fail_at(-1);
        CHECK(big(g) == hipSuccess && recorded(g));
    }
    for (long k = 0;; ++k) { // grown from a smaller job: the k-th allocation of the growth fails
        G g;
        fail_at(-1);
        CHECK(small(g) == hipSuccess);
        fail_at(k);
        const hipError_t e = big(g);
        if (e == hipSuccess) { CHECK(recorded(g)); break; }
        CHECK(e == hipErrorOutOfMemory && empty(g) && g_live.empty());
    }
    fail_at(-1);
    CHECK(g_live.empty());
    printf("  %s: %ld allocations, each failure leaves the group empty\n", what, n_alloc);
}

void case_groups()
{
    every_failure<JobBufs>("job twins", [](JobBufs& g) { return g.ensure(10); }, [](JobBufs& g) { return g.ensure(5000); });
    every_failure<HashBufs>("hashing", [](HashBufs& g) { return g.ensure(4, true, 4); }, [](HashBufs& g) { return g.ensure(100, true, 2000); });
    every_failure<Twin<CmpChunk>>("compare", [](Twin<CmpChunk>& g) { return g.ensure(8192); }, [](Twin<CmpChunk>& g) { return g.ensure(20000); });
    every_failure<Slot>("staging slot", [](Slot& g) { return g.ensure(1 << 16, 0); }, [](Slot& g) { return g.ensure(1 << 20, 0); });
    every_failure<DeflateBufs>("deflate", [](DeflateBufs& g) { return g.ensure(128, 1); }, [](DeflateBufs& g) { return g.ensure(1024, 1); });
    every_failure<InflateBufs>("inflate", [](InflateBufs& g) { return g.ensure(1 << 16, 64, -1); }, [](InflateBufs& g) { return g.ensure(8 << 20, 512, -1); });
    every_failure<Bzip2Bufs>("bzip2", [](Bzip2Bufs& g) { return g.ensure(1 << 16, 8, 0); }, [](Bzip2Bufs& g) { return g.ensure(4 << 20, 16, 0); });

    // a group's each() lists every buffer: the footprint of a sized DEFLATE group is what its ensure() asked for
    DeflateBufs z;
    CHECK(z.ensure(100, 0) == hipSuccess && z.chunks() == 100);
    Footprint f;
    z.each(f);
    CHECK(f.hbm == 100ull * (2 * kDeflateSlot + 4 * kDeflateTokWords + 4 + 8));
    CHECK(f.pinned == 100ull * (4 + 8 + 2 * kDeflateSlot));
    CHECK(f.hbm + f.pinned == live_bytes());
    z.each(Release());
    CHECK(empty(z) && g_live.empty());
    printf("groups ok\n");
}

// The review's sequence (targz.inc GzipEncoder::ensure): a small job's ensure fails after its first buffer,
// then a larger job's ensure succeeds on the same group.  Every buffer must hold the larger job.
void case_review()
{
    constexpr size_t kBig = 4096;
    {
        DeflateBufs z;
        fail_at(1);
        CHECK(z.ensure(128, 0) == hipErrorOutOfMemory && empty(z));
        fail_at(-1);
        CHECK(z.ensure(kBig, 0) == hipSuccess && z.chunks() == kBig && recorded(z));
        CHECK(z.d_slots.size() >= kBig * kDeflateSlot && z.d_out.size() >= kBig * kDeflateSlot);
        CHECK(z.d_toks.size() >= kBig * kDeflateTokWords);
        CHECK(z.d_sizes.size() >= kBig && z.d_prefix.size() >= kBig && z.h_sizes.size() >= kBig && z.h_prefix.size() >= kBig);
        CHECK(z.h_out[0].size() >= kBig * kDeflateSlot && z.h_out[1].size() >= kBig * kDeflateSlot);
    }
    {
        constexpr uint64_t kPiece = 64ull << 20;
        constexpr uint32_t kSlots = 512;
        InflateBufs f;
        fail_at(1);
        CHECK(f.ensure(1 << 20, 64, 0) == hipErrorOutOfMemory && empty(f));
        fail_at(-1);
        CHECK(f.ensure(kPiece, kSlots, 0) == hipSuccess && recorded(f));
        CHECK(f.d_in.size() >= kPiece + 16 && f.cand_cap() == kPiece / 4 + 16 && f.h_cand.size() >= f.cand_cap() + 2);
        CHECK(f.nslots() == kSlots && f.d_slots.size() >= (size_t)kSlots * kInflateSlotSyms);
        CHECK(f.h_res.size() >= kSlots && f.d_links.size() >= kSlots && f.h_links.size() >= kSlots);
        CHECK(f.d_flags.size() >= 4 && f.h_flags.size() >= 4 && f.d_win.size() >= kInfWindow && f.d_out.size() == 0);
    }
    {
        constexpr uint64_t kPiece = 64ull << 20;
        constexpr uint32_t kSlots = 16;
        Bzip2Bufs b;
        fail_at(1);
        CHECK(b.ensure(1 << 20, 8, 0) == hipErrorOutOfMemory && empty(b));
        fail_at(-1);
        CHECK(b.ensure(kPiece, kSlots, 0) == hipSuccess && recorded(b));
        CHECK(b.d_in.size() >= kPiece + 16 && b.cand_cap() == bz_candidate_cap(kPiece) && b.h_cand.size() >= b.cand_cap());
        CHECK(b.nslots() == kSlots && b.d_slots.size() >= (size_t)kSlots * kBzMaxBlock && b.d_tt.size() >= (size_t)kSlots * kBzMaxBlock);
        CHECK(b.d_chunks.size() >= (size_t)kSlots * kBzChunks && b.h_res.size() >= kSlots && b.d_blk.size() >= kSlots && b.h_blk.size() >= kSlots);
        CHECK(b.d_count.size() >= 4 && b.h_count.size() >= 4);
    }
    CHECK(g_live.empty());
    printf("review ok\n");
}

} // namespace

hipError_t snaphash::devbuf_alloc(Mem kind, void** p, size_t bytes, int numa_node)
{
    *p = nullptr;
    if (g_calls++ == g_fail_at) return hipErrorOutOfMemory;
    *p = malloc(bytes ? bytes : 1);
    if (!*p) return hipErrorOutOfMemory;
    g_live[*p] = Block{kind, bytes, numa_node};
    return hipSuccess;
}

void snaphash::devbuf_free(Mem kind, void* p)
{
    auto it = g_live.find(p);
    CHECK(it != g_live.end() && it->second.kind == kind); // freed once, by its own kind
    g_live.erase(it);
    free(p);
}

int main(int argc, char** argv)
{
    const std::string c = argc > 1 ? argv[1] : "all";
    if (c == "buf" || c == "all") case_buf();
    if (c == "groups" || c == "all") case_groups();
    if (c == "review" || c == "all") case_review();
    if (c == "all") printf("all ok\n");
    return 0;
}
