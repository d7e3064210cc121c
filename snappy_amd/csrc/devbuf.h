// devbuf.h -- an owning, typed buffer of HBM or pinned host memory whose pointer and size always agree.  Internal.
//
// The header allocates nothing itself: it calls devbuf_alloc / devbuf_free, which the library defines once
// (snaphash_api.cpp: hipMalloc, and pinned memory on a NUMA node) and a CPU test defines with fakes.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace snaphash {

enum class Mem { Hbm, Pinned };

// numa_node applies to Mem::Pinned: the node the pages are placed on, -1 for wherever the runtime puts them
hipError_t devbuf_alloc(Mem kind, void** p, size_t bytes, int numa_node);
void devbuf_free(Mem kind, void* p);

template <class T, Mem K>
class Buf {
public:
    Buf() = default;
    Buf(Buf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    Buf& operator=(Buf&& o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = o.p_; n_ = o.n_;
            o.p_ = nullptr; o.n_ = 0;
        }
        return *this;
    }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { reset(); }

    T* data() const { return p_; }
    size_t size() const { return n_; } // elements
    uint64_t bytes() const { return (uint64_t)n_ * sizeof(T); }
    T& operator[](size_t i) const
    {
        static_assert(K == Mem::Pinned, "HBM is not read through a host pointer");
        return p_[i];
    }

    void reset()
    {
        if (p_) devbuf_free(K, p_);
        p_ = nullptr;
        n_ = 0;
    }
    // n elements at least: a buffer that holds them is kept; a smaller one is freed before the new one is allocated.
    // On failure the buffer is empty.
    hipError_t reserve(size_t n)
    {
        static_assert(K == Mem::Hbm, "pinned memory: reserve(n, numa_node)");
        return grow(n, -1);
    }
    hipError_t reserve(size_t n, int numa_node)
    {
        static_assert(K == Mem::Pinned, "HBM: reserve(n)");
        return grow(n, numa_node);
    }

private:
    hipError_t grow(size_t n, int node)
    {
        if (n <= n_) return hipSuccess;
        reset();
        void* p = nullptr;
        const hipError_t e = devbuf_alloc(K, &p, n * sizeof(T), node);
        if (e != hipSuccess) return e;
        p_ = (T*)p;
        n_ = n;
        return hipSuccess;
    }
    T* p_ = nullptr;
    size_t n_ = 0;
};

template <class T> using DevBuf = Buf<T, Mem::Hbm>;
template <class T> using HostBuf = Buf<T, Mem::Pinned>;

// Visitors for a group's each(): what its buffers hold, by kind, and their release.
struct Footprint {
    uint64_t pinned = 0, hbm = 0;
    template <class T, Mem K> void operator()(const Buf<T, K>& b) { (K == Mem::Pinned ? pinned : hbm) += b.bytes(); }
};
struct Release {
    template <class T, Mem K> void operator()(Buf<T, K>& b) { b.reset(); }
};

} // namespace snaphash
