// The host CRC routines the decoders use (DESIGN.md sec. 16's yardstick for the CRC kernels), timed on 64 MiB of random
// bytes: gzip's CRC-32 as crc_parallel takes it (targz.inc: 4 MiB ranges on four threads of tarpack.cpp's crc32_update,
// combined in order) and on one thread; bzip2's bz_crc_block (bzip2_host.cpp) on one thread and on 16 (a sixteenth
// each, as bunzip2_batch deals blocks to threads).  One JSON line.
// build: g++ -O3 -std=c++17 -o tools/crc_host_bench tools/crc_host_bench.cpp snappy_amd/csrc/tarpack.o snappy_amd/csrc/walk.o
//        snappy_amd/csrc/hostfill.o snappy_amd/csrc/bzip2_host.o -pthread   (after make -C snappy_amd/csrc)
#include <stdio.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <random>
#include <thread>
#include <vector>

#include "../snappy_amd/csrc/bzip2_host.h"
#include "../snappy_amd/csrc/tarpack.h"

using namespace snaphash;

static double now_ms()
{
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

template <class F> static double best(F&& f, int reps = 5)
{
    double b = 1e30;
    for (int i = 0; i < reps; ++i) {
        const double t0 = now_ms();
        f();
        b = std::min(b, now_ms() - t0);
    }
    return b;
}

static uint32_t gz_parallel(const uint8_t* p, size_t n, unsigned T)
{
    const size_t kRange = 4u << 20, nr = (n + kRange - 1) / kRange;
    std::vector<uint32_t> part(nr);
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (size_t i; (i = next.fetch_add(1)) < nr;) part[i] = crc32_update(0, p + i * kRange, std::min(kRange, n - i * kRange));
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < T; ++t) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
    uint32_t crc = part[0];
    for (size_t i = 1; i < nr; ++i) crc = crc32_combine(crc, part[i], std::min(kRange, n - i * kRange));
    return crc;
}

int main()
{
    const size_t n = 64u << 20;
    std::vector<uint8_t> buf(n);
    std::mt19937_64 g(1);
    for (size_t i = 0; i < n; i += 8) *(uint64_t*)&buf[i] = g();
    volatile uint32_t sink = 0;
    const double gz1 = best([&] { sink = crc32_update(0, buf.data(), n); });
    const double gz4 = best([&] { sink = gz_parallel(buf.data(), n, 4); });
    const double bz1 = best([&] { sink = bz_crc_block(buf.data(), n); }, 2);
    const double bz16 = best([&] {
        std::vector<std::thread> th;
        for (int t = 0; t < 16; ++t) th.emplace_back([&, t] { sink = bz_crc_block(buf.data() + (size_t)t * (n / 16), n / 16); });
        for (auto& t : th) t.join();
    }, 3);
    auto gbps = [&](double ms) { return n / ms / 1e6; };
    printf("{\"leg\": \"host_crc\", \"bytes\": %zu, \"crc32_one_thread_ms\": %.2f, \"crc32_one_thread_gbps\": %.2f, \"crc_parallel_4_threads_ms\": %.2f, "
           "\"crc_parallel_4_threads_gbps\": %.2f, \"bz_crc_block_one_thread_ms\": %.1f, \"bz_crc_block_one_thread_gbps\": %.3f, "
           "\"bz_crc_block_16_threads_ms\": %.1f, \"bz_crc_block_16_threads_gbps\": %.2f}\n",
           n, gz1, gbps(gz1), gz4, gbps(gz4), bz1, gbps(bz1), bz16, gbps(bz16));
    (void)sink;
    return 0;
}
