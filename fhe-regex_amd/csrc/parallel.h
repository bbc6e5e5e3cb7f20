// fn(i) for 0 <= i < n on up to 16 host threads, index i on thread i % T; returns when all are done.
#pragma once
#include <thread>
#include <vector>

namespace fr {

template <class F>
static void parallel_for(int n, F&& fn) {
    unsigned hw = std::thread::hardware_concurrency();
    int T = (int)(hw ? (hw > 16 ? 16 : hw) : 4);
    if (T > n) T = n > 0 ? n : 1;
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t)
        th.emplace_back([&, t] {
            for (int i = t; i < n; i += T) fn(i);
        });
    for (auto& x : th) x.join();
}

}  // namespace fr
