// Stand-alone check of the step schedule (fhe-regex_amd/csrc/step_sched.h): the entry packing
// and the table's build by the helpers the blind rotation's prologue itself calls (rank_below,
// entry_of); only the live masks, a wave ballot on the device, are formed by a plain loop here.
// For random and edge masks, walking the table visits exactly the non-idle steps in order with
// their pairs, and ends at the end entry.  For an ASan + UBSan build, CPU only:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iinclude -Ifhe-regex_amd/csrc tools/step_sched_check.cpp -o /tmp/step_sched_check && /tmp/step_sched_check
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

#include "step_sched.h"

using namespace fr;

// the prologue's build for B bootstraps of n mask elements each (abar[b][n + 1], zero-padded)
static std::vector<uint64_t> build(const std::vector<std::vector<uint16_t>>& abar, int steps) {
    const int B = (int)abar.size();
    auto idle = [&](int t) {
        uint32_t z = 0;
        for (int b = 0; b < B; ++b) z |= abar[b][2 * t] | abar[b][2 * t + 1];
        return z == 0;
    };
    std::vector<uint64_t> live(step_sched::MAX_STEPS / 64, 0), sched(steps + 1, ~0ULL);
    for (int t = 0; t < steps; ++t)
        if (!idle(t)) live[t >> 6] |= 1ULL << (t & 63);
    // the kernel's layout: bootstrap b's elements at flat + b * stride
    const int stride = 2 * steps + 2;
    std::vector<uint16_t> flat((size_t)B * stride);
    for (int b = 0; b < B; ++b) std::copy(abar[b].begin(), abar[b].end(), flat.begin() + (size_t)b * stride);
    for (int t = 0; t <= steps; ++t) {
        const int rank = step_sched::rank_below(live.data(), t);
        if (t == steps) sched.at(rank) = step_sched::END_ENTRY;
        else if (!idle(t))
            sched.at(rank) = B == 1 ? step_sched::entry_of<1>(flat.data(), stride, t) : step_sched::entry_of<2>(flat.data(), stride, t);
    }
    return sched;
}

static int check(const std::vector<std::vector<uint16_t>>& abar, int steps) {
    const std::vector<uint64_t> sched = build(abar, steps);
    const int B = (int)abar.size();
    size_t i = 0;
    for (int t = 0; t < steps; ++t) {
        bool any = false;
        for (int b = 0; b < B; ++b) any |= abar[b][2 * t] || abar[b][2 * t + 1];
        if (!any) continue;
        const uint64_t e = sched.at(i++);
        if ((int)step_sched::step(e) != t) return 1;
        for (int b = 0; b < B; ++b)
            if (step_sched::pair_i(e, b) != abar[b][2 * t] || step_sched::pair_j(e, b) != abar[b][2 * t + 1]) return 1;
    }
    return step_sched::step(sched.at(i)) == step_sched::END ? 0 : 1;
}

int main() {
    std::mt19937_64 rng(7);
    int bad = 0, cases = 0;
    for (int B = 1; B <= 2; ++B)
        for (int n : {1, 2, 63, 64, 127, 128, 129, 741, 742, 1023, 1024})
            for (int density : {0, 1, 50, 99, 100})
                for (int rep = 0; rep < 4; ++rep) {
                    const int steps = (n + 1) / 2;
                    std::vector<std::vector<uint16_t>> abar(B, std::vector<uint16_t>(2 * steps + 2, 0));
                    for (int b = 0; b < B; ++b)
                        for (int t = 0; t < steps; ++t)
                            if ((int)(rng() % 100) < density) {
                                abar[b][2 * t] = (uint16_t)(rng() % 4096);
                                if (2 * t + 1 < n) abar[b][2 * t + 1] = rep & 1 ? 4095 : (uint16_t)(rng() % 4096);
                            }
                    bad += check(abar, steps);
                    ++cases;
                }
    std::printf("step_sched_check: %d cases, %d bad\n", cases, bad);
    return bad != 0;
}
