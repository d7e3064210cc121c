// Test-only (CPU): the engine's owning events and streams, its ledger of timed spans and its stage timer
// (snappy_amd/csrc/gpu_handles.h) against fake hooks that record every live handle and can fail their k-th creation.  The
// library defines gpu_event_create and the other three with the runtime's calls; here a handle is a number.  The stage
// timer's two runtime calls, hipEventRecord and hipEventElapsedTime, are fakes too: a mark writes down its event, a time
// is the distance between two events' numbers.  Not part of the product.
//
// usage: gpu_handles_host <case>   (handles | ledger | clock | all); prints "<case> ok" and exits 0, or the first failure and 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <set>
#include <string>
#include <vector>

#include "../snappy_amd/csrc/gpu_handles.h"

using namespace snaphash;

namespace {

std::set<uintptr_t> g_events, g_streams; // live
std::map<uintptr_t, unsigned> g_flags;   // what a live handle was created with
std::map<uintptr_t, int> g_priority;
uintptr_t g_next = 0x1000;
long g_created = 0;  // creations asked for so far, events and streams alike
long g_fail_at = -1; // the creation (0-based) that fails; -1: none
std::vector<uintptr_t> g_marks; // events recorded, in order

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

void fail_at(long k) { g_created = 0; g_fail_at = k; }
size_t live() { return g_events.size() + g_streams.size(); }
bool live_event(hipEvent_t e) { return g_events.count((uintptr_t)e) != 0; }

void case_handles()
{
    fail_at(-1);
    {
        Event e;
        CHECK(e.get() == nullptr && !e && live() == 0);
        e.reset(); // empty: nothing to destroy
        CHECK(e.ensure(hipEventDisableTiming) == hipSuccess && e.get() && live_event(e.get()) && g_flags.at((uintptr_t)e.get()) == hipEventDisableTiming);
        const hipEvent_t raw = e.get();
        CHECK(e.ensure() == hipSuccess && e.get() == raw && g_created == 1); // full: kept, nothing created
        CHECK((hipEvent_t)e == raw);
        Event f(std::move(e)); // move construction: the handle changes hands
        CHECK(e.get() == nullptr && f.get() == raw && live() == 1);
        Event g;
        CHECK(g.ensure() == hipSuccess && live() == 2 && g_flags.at((uintptr_t)g.get()) == hipEventDefault);
        g = std::move(f); // move assignment onto a full handle: g's own goes
        CHECK(g.get() == raw && f.get() == nullptr && live() == 1 && live_event(raw));
        Event& same = g;
        g = std::move(same); // self-move: kept
        CHECK(g.get() == raw && live() == 1);
        g.reset();
        CHECK(g.get() == nullptr && live() == 0);
        g.reset();
        fail_at(0);
        CHECK(g.ensure() == hipErrorOutOfMemory && g.get() == nullptr && live() == 0); // a failed creation leaves it empty
        fail_at(-1);
        CHECK(g.ensure() == hipSuccess && live() == 1);
    }
    CHECK(live() == 0); // the destructor
    {
        Stream s, p;
        CHECK(s.ensure(hipStreamNonBlocking) == hipSuccess && g_priority.at((uintptr_t)s.get()) == kStreamDefaultPriority);
        CHECK(p.ensure(hipStreamNonBlocking, 3) == hipSuccess && g_priority.at((uintptr_t)p.get()) == 3 && g_flags.at((uintptr_t)p.get()) == hipStreamNonBlocking);
        const hipStream_t raw = s.get();
        CHECK(s.ensure(hipStreamNonBlocking, 1) == hipSuccess && s.get() == raw && live() == 2);
        Stream t(std::move(s));
        p = std::move(t);
        CHECK(p.get() == raw && s.get() == nullptr && t.get() == nullptr && live() == 1);
        Stream& same = p;
        p = std::move(same);
        CHECK(p.get() == raw && live() == 1);
    }
    CHECK(live() == 0);
    { // a caller's stream: used, never destroyed, through every way a handle ends
        const hipStream_t callers = (hipStream_t)(uintptr_t)0x77;
        const long before = g_created;
        Stream a;
        a.adopt(callers);
        CHECK(a.get() == callers && a.ensure(hipStreamNonBlocking) == hipSuccess && a.get() == callers && g_created == before);
        Stream b(std::move(a));
        Stream c;
        CHECK(c.ensure(hipStreamNonBlocking) == hipSuccess && live() == 1);
        c = std::move(b); // c's own goes, the adopted one arrives as adopted
        CHECK(c.get() == callers && live() == 0);
        c.reset();
        CHECK(c.get() == nullptr);
        CHECK(c.ensure(hipStreamNonBlocking) == hipSuccess && live() == 1); // and an emptied handle owns what it creates next
        c.adopt(callers); // adopting over an owned stream destroys that one
        CHECK(live() == 0);
        Stream d;
        d.adopt(callers);
    } // (the fake destroy refuses a handle it did not create)
    CHECK(live() == 0);
    printf("handles ok\n");
}

void case_ledger()
{
    fail_at(-1);
    {
        EventLedger l;
        Span first, s;
        CHECK(l.used() == 0 && l.take(Ev::H2d, &first) == hipSuccess && first.a && first.b && first.a != first.b);
        for (int i = 1; i < 1000; ++i) CHECK(l.take(Ev::Codec, &s) == hipSuccess); // growth moves the storage, not the handles
        CHECK(l.used() == 1000 && live() == 2000 && live_event(first.a) && live_event(first.b));
        std::vector<Span> seen;
        l.each([&](Ev, const Span& sp) { seen.push_back(sp); });
        CHECK(seen.size() == 1000 && seen[0].a == first.a && seen[0].b == first.b && seen[999].a == s.a && seen[999].b == s.b);
        l.clear(); // the events are kept: a second call of the same shape creates none
        const long created = g_created;
        CHECK(l.used() == 0 && live() == 2000);
        for (int i = 0; i < 1000; ++i) {
            CHECK(l.take(Ev::Hash, &s) == hipSuccess);
            if (i == 0) CHECK(s.a == first.a && s.b == first.b);
        }
        CHECK(g_created == created && l.used() == 1000 && live() == 2000);
        CHECK(l.take(Ev::Hash, &s) == hipSuccess && g_created == created + 2); // growth alone creates
    }
    CHECK(live() == 0);

    // every creation of a run of 8 takes fails in turn: whole pairs only, used() at what succeeded, nothing left behind
    long n_created;
    {
        EventLedger l;
        Span s;
        fail_at(-1);
        for (int i = 0; i < 8; ++i) CHECK(l.take(Ev::Check, &s) == hipSuccess);
        n_created = g_created;
    }
    CHECK(n_created == 16 && live() == 0);
    for (long k = 0; k < n_created; ++k) {
        {
            EventLedger l;
            Span s;
            fail_at(k);
            size_t ok = 0;
            for (int i = 0; i < 8; ++i) {
                const hipError_t e = l.take(Ev::Check, &s);
                if (e == hipSuccess) { ++ok; continue; }
                CHECK(e == hipErrorOutOfMemory && (size_t)i == (size_t)k / 2);
                break;
            }
            CHECK(ok == (size_t)k / 2 && l.used() == ok && live() == 2 * ok);
            size_t visited = 0;
            l.each([&](Ev kind, const Span& sp) { CHECK(kind == Ev::Check && live_event(sp.a) && live_event(sp.b)); ++visited; });
            CHECK(visited == ok);
            fail_at(-1);
            CHECK(l.take(Ev::Check, &s) == hipSuccess && l.used() == ok + 1 && live() == 2 * ok + 2); // and it goes on
        }
        CHECK(live() == 0);
    }

    // visiting: kinds in take order, and a sum by kind over a mixed sequence with the test's own times
    {
        EventLedger l;
        const Ev kinds[] = {Ev::H2d, Ev::Hash, Ev::Codec, Ev::Codec, Ev::Check, Ev::H2d, Ev::Hash, Ev::Codec, Ev::Check, Ev::H2d};
        const float times[] = {1, 2, 4, 8, 16, 32, 64, 128, 256, 512};
        std::map<hipEvent_t, float> ms_of;
        for (int i = 0; i < 10; ++i) {
            Span s;
            CHECK(l.take(kinds[i], &s) == hipSuccess);
            ms_of[s.a] = times[i];
        }
        int i = 0;
        l.each([&](Ev kind, const Span&) { CHECK(kind == kinds[i]); ++i; });
        CHECK(i == 10);
        const SpanSums all = sum_spans(l, [&](const Span& s, float* ms) { *ms = ms_of.at(s.a); return true; });
        CHECK(all.h2d == 1 + 32 + 512 && all.hash == 2 + 64 && all.codec == 4 + 8 + 128 && all.check == 16 + 256);
        // a span whose time is not known counts nothing
        const SpanSums some = sum_spans(l, [&](const Span& s, float* ms) { *ms = ms_of.at(s.a); return *ms != 8 && *ms != 512; });
        CHECK(some.h2d == 1 + 32 && some.hash == 2 + 64 && some.codec == 4 + 128 && some.check == 16 + 256);
        l.clear();
        const SpanSums none = sum_spans(l, [&](const Span&, float* ms) { *ms = 1000; return true; });
        CHECK(none.h2d == 0 && none.hash == 0 && none.codec == 0 && none.check == 0);
    }
    CHECK(live() == 0);
    printf("ledger ok\n");
}

void case_clock()
{
    const hipStream_t s = (hipStream_t)(uintptr_t)0x55;
    fail_at(-1);
    {
        StageClock<4> off; // disabled: nothing created, marks succeed and record nothing
        g_marks.clear();
        for (int i = 0; i <= 4; ++i) CHECK(off.mark(i, s) == hipSuccess);
        CHECK(!off.enabled() && off.raw() == nullptr && off.ms(0) == 0 && g_created == 0 && live() == 0 && g_marks.empty());
    }
    for (long k = 0; k < 5; ++k) { // a failure at each creation leaves none behind, and the clock disabled
        StageClock<4> c;
        fail_at(k);
        CHECK(c.enable() == hipErrorOutOfMemory && !c.enabled() && c.raw() == nullptr && live() == 0);
        CHECK(c.mark(0, s) == hipSuccess);
        fail_at(-1);
        CHECK(c.enable() == hipSuccess && c.enabled() && live() == 5);
    }
    CHECK(live() == 0);
    fail_at(-1);
    {
        StageClock<2> c;
        CHECK(c.enable() == hipSuccess && g_created == 3 && c.enable() == hipSuccess && g_created == 3);
        hipEvent_t* raw = c.raw();
        CHECK(raw && live_event(raw[0]) && live_event(raw[1]) && live_event(raw[2]));
        g_marks.clear();
        for (int i = 0; i <= 2; ++i) CHECK(c.mark(i, s) == hipSuccess);
        CHECK(g_marks.size() == 3 && g_marks[0] == (uintptr_t)raw[0] && g_marks[1] == (uintptr_t)raw[1] && g_marks[2] == (uintptr_t)raw[2]);
        // (the fake time between two events is the distance of their numbers)
        CHECK(c.ms(0) == (float)((uintptr_t)raw[1] - (uintptr_t)raw[0]) && c.ms(1) == (float)((uintptr_t)raw[2] - (uintptr_t)raw[1]));
    }
    CHECK(live() == 0);
    printf("clock ok\n");
}

uintptr_t create(std::set<uintptr_t>& into, unsigned flags)
{
    if (g_created++ == g_fail_at) return 0;
    const uintptr_t h = g_next += 0x10;
    into.insert(h);
    g_flags[h] = flags;
    return h;
}

void destroy(std::set<uintptr_t>& from, uintptr_t h)
{
    CHECK(from.erase(h) == 1); // created here, destroyed once, by its own kind
    g_flags.erase(h);
    g_priority.erase(h);
}

} // namespace

hipError_t snaphash::gpu_event_create(hipEvent_t* e, unsigned flags)
{
    const uintptr_t h = create(g_events, flags);
    if (!h) return hipErrorOutOfMemory;
    *e = (hipEvent_t)h;
    return hipSuccess;
}
void snaphash::gpu_event_destroy(hipEvent_t e) { destroy(g_events, (uintptr_t)e); }
hipError_t snaphash::gpu_stream_create(hipStream_t* s, unsigned flags, int priority)
{
    const uintptr_t h = create(g_streams, flags);
    if (!h) return hipErrorOutOfMemory;
    g_priority[h] = priority;
    *s = (hipStream_t)h;
    return hipSuccess;
}
void snaphash::gpu_stream_destroy(hipStream_t s) { destroy(g_streams, (uintptr_t)s); }

extern "C" hipError_t hipEventRecord(hipEvent_t e, hipStream_t)
{
    CHECK(live_event(e));
    g_marks.push_back((uintptr_t)e);
    return hipSuccess;
}
extern "C" hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b)
{
    CHECK(live_event(a) && live_event(b));
    *ms = (float)((uintptr_t)b - (uintptr_t)a);
    return hipSuccess;
}

int main(int argc, char** argv)
{
    const std::string c = argc > 1 ? argv[1] : "all";
    if (c == "handles" || c == "all") case_handles();
    if (c == "ledger" || c == "all") case_ledger();
    if (c == "clock" || c == "all") case_clock();
    if (c == "all") printf("all ok\n");
    return 0;
}
