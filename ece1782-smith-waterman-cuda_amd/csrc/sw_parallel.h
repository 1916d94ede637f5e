// sw_parallel.h — the host code's one thread pool shape: a loop over indices
// shared out to a few threads (sw_db.cpp's copies and staged uploads,
// sw_pack.cpp's lane tables).  No HIP.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>

namespace swk {

inline int default_threads() {
    unsigned n = std::thread::hardware_concurrency();
    if (n == 0) n = 4;
    return static_cast<int>(std::min(16u, n));  // GPU boxes expose many more CPUs than our share
}

// f(i) for i in [0, n) on up to default_threads() threads, `grain` indices
// per grab (at least one grab per thread).
template <class F>
void parallel_for(int64_t n, F&& f, int64_t grain = 64) {
    const int nt = static_cast<int>(std::min<int64_t>(default_threads(), std::max<int64_t>(1, n / grain)));
    if (nt <= 1) {
        for (int64_t i = 0; i < n; ++i) f(i);
        return;
    }
    std::atomic<int64_t> next{0};
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t)
        th.emplace_back([&] {
            for (;;) {
                const int64_t i0 = next.fetch_add(grain);
                if (i0 >= n) break;
                const int64_t i1 = std::min(n, i0 + grain);
                for (int64_t i = i0; i < i1; ++i) f(i);
            }
        });
    for (auto& t : th) t.join();
}

}  // namespace swk
