// gpu_handles.h -- owning HIP events and streams, the ledger of an engine's timed spans, and a stage timer.  Internal.
//
// Like devbuf.h the header creates nothing itself: it calls gpu_event_create / gpu_event_destroy / gpu_stream_create /
// gpu_stream_destroy, which the library defines once (snaphash_api.cpp) and a CPU test defines with fakes.  StageClock
// alone records and reads its events with the runtime's own hipEventRecord and hipEventElapsedTime.
#pragma once
#include <hip/hip_runtime_api.h>
#include <limits.h>
#include <stddef.h>

#include <utility>
#include <vector>

namespace snaphash {

constexpr int kStreamDefaultPriority = INT_MIN; // gpu_stream_create: a stream of the runtime's default priority

hipError_t gpu_event_create(hipEvent_t* e, unsigned flags);
void gpu_event_destroy(hipEvent_t e);
hipError_t gpu_stream_create(hipStream_t* s, unsigned flags, int priority);
void gpu_stream_destroy(hipStream_t s);

// One handle, move-only, empty by default.  It converts to the raw handle, so the runtime's calls take it as it stands.
// A handle learns how it is destroyed where it is created: code that only holds empty ones (a CPU test of the buffer
// groups in engine_bufs.h) needs none of the hooks.
template <class H>
class Handle {
public:
    Handle() = default;
    Handle(Handle&& o) noexcept : h_(o.h_), destroy_(o.destroy_) { o.h_ = nullptr; }
    Handle& operator=(Handle&& o) noexcept
    {
        if (this != &o) { reset(); h_ = o.h_; destroy_ = o.destroy_; o.h_ = nullptr; }
        return *this;
    }
    Handle(const Handle&) = delete;
    Handle& operator=(const Handle&) = delete;
    ~Handle() { reset(); }

    H get() const { return h_; }
    operator H() const { return h_; }
    void reset() { if (h_ && destroy_) destroy_(h_); h_ = nullptr; }

protected:
    // a handle that `create` made is owned, and `destroy` ends it; on failure the handle stays empty
    template <class Create> hipError_t ensure_with(Create create, void (*destroy)(H))
    {
        if (h_) return hipSuccess;
        H h = nullptr;
        const hipError_t e = create(&h);
        if (e == hipSuccess) { h_ = h; destroy_ = destroy; }
        return e;
    }
    H h_ = nullptr;
    void (*destroy_)(H) = nullptr; // null: empty, or a handle that is not ours to destroy
};

struct Event : Handle<hipEvent_t> {
    // created on first use; a full handle is kept, whatever its flags
    hipError_t ensure(unsigned flags = hipEventDefault) { return ensure_with([&](hipEvent_t* e) { return gpu_event_create(e, flags); }, gpu_event_destroy); }
};

struct Stream : Handle<hipStream_t> {
    hipError_t ensure(unsigned flags, int priority = kStreamDefaultPriority) { return ensure_with([&](hipStream_t* s) { return gpu_stream_create(s, flags, priority); }, gpu_stream_destroy); }
    // a caller's stream (snaphash_config.stream): used, never destroyed
    void adopt(hipStream_t s) { reset(); h_ = s; destroy_ = nullptr; }
};

enum class Ev { Hash, H2d, Codec, Check }; // what a span times: SHA-512 kernels; staging copies; any codec's, CRC's or SHA-256's launch; a self-check
struct Span { hipEvent_t a = nullptr, b = nullptr; }; // recorded before and after what it times

// The timed spans of an engine's call, in the order they were taken.  Two uses: a call that reports event times at its
// end takes its spans and sums them by kind once its streams have drained (collect_events); a call that reads each span
// where it ends uses the pairs as scratch and clears them unread.  clear() keeps the events, so a second call of the
// same shape creates none.  take() hands the handles out by value and they stay valid for the ledger's life: nothing
// outside holds a pointer into its storage.
// One thread at a time: only the thread that runs the engine's call takes, visits and clears (the asynchronous fill of
// tar_create_impl is handed its span by value and takes none itself), so there is no lock.
class EventLedger {
public:
    hipError_t take(Ev kind, Span* out)
    {
        if (used_ == pairs_.size()) {
            Pair p;
            hipError_t e = p.a.ensure();
            if (e == hipSuccess) e = p.b.ensure();
            if (e != hipSuccess) return e; // (whole pairs only: p's first event dies here)
            pairs_.push_back(std::move(p));
        }
        Pair& p = pairs_[used_++];
        p.kind = kind;
        *out = Span{p.a.get(), p.b.get()};
        return hipSuccess;
    }
    size_t used() const { return used_; }
    void clear() { used_ = 0; }
    // f(kind, span) for every span taken since the last clear(), in take order
    template <class F> void each(F&& f) const { for (size_t i = 0; i < used_; ++i) f(pairs_[i].kind, Span{pairs_[i].a.get(), pairs_[i].b.get()}); }

private:
    struct Pair { Event a, b; Ev kind = Ev::Hash; };
    std::vector<Pair> pairs_;
    size_t used_ = 0;
};

// What a ledger's spans took, by kind: sum_spans(ledger, elapsed) with elapsed(span, &ms) -> whether ms is known.
struct SpanSums { double hash = 0, h2d = 0, codec = 0, check = 0; };
template <class Elapsed> SpanSums sum_spans(const EventLedger& l, Elapsed elapsed)
{
    SpanSums s;
    l.each([&](Ev kind, const Span& sp) {
        float ms = 0;
        if (!elapsed(sp, &ms)) return;
        (kind == Ev::Hash ? s.hash : kind == Ev::H2d ? s.h2d : kind == Ev::Codec ? s.codec : s.check) += ms;
    });
    return s;
}

// N stages between N + 1 marks on a stream, for trace lines and calibration.  Disabled (the default) it owns no event
// and mark() does nothing; enable() creates all of them or none.
template <int N>
class StageClock {
public:
    hipError_t enable()
    {
        hipError_t r = hipSuccess;
        for (Event& e : ev_) if (r == hipSuccess) r = e.ensure();
        for (int i = 0; i <= N; ++i) { if (r != hipSuccess) ev_[i].reset(); raw_[i] = ev_[i].get(); }
        return r;
    }
    bool enabled() const { return raw_[0] != nullptr; }
    hipError_t mark(int i, hipStream_t s) { return enabled() ? hipEventRecord(raw_[i], s) : hipSuccess; }
    float ms(int i) const { float t = 0; return enabled() && hipEventElapsedTime(&t, raw_[i], raw_[i + 1]) == hipSuccess ? t : 0; } // marks i .. i + 1; 0: not known
    hipEvent_t* raw() { return enabled() ? raw_ : nullptr; } // the N + 1 events, for a launcher that records them itself

private:
    Event ev_[N + 1];
    hipEvent_t raw_[N + 1] = {};
};

} // namespace snaphash
