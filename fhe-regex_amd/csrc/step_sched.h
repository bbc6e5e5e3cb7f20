// The blind rotation's packed step schedule (fft_br.hip, fbr_rotate, k = 1): one 64-bit entry per
// unskipped step, in order, closed by an end entry.  An entry holds 12-bit fields: field 0 the
// step index t, fields 1 + 2b and 2 + 2b the mod-switched pair (e_i, e_j) of bootstrap b of the
// workgroup (pair shape: b < 2, 60 bits in all).  The end entry has t = END, which no step
// reaches (t < 512).  The rotation builds the table in LDS once, in its prologue, and walks it
// one entry ahead, so a step finds its index and pairs in scalar registers.
#pragma once
#include "common.h"

namespace fr {
namespace step_sched {

constexpr int FIELD_BITS = 12, FIELDS = 5;
constexpr uint32_t FIELD_MASK = (1u << FIELD_BITS) - 1;
constexpr uint32_t END = FIELD_MASK;  // field 0 of the entry after the last unskipped step
constexpr int MAX_STEPS = 512;        // steps of a rotation (n <= 1024): entries <= MAX_STEPS + 1
static_assert(FIELDS * FIELD_BITS <= 64 && MAX_STEPS <= (int)END, "five fields in 64 bits, END above every step");

// entry e with field f (zero before) set to v < 2^12
FR_HD constexpr uint64_t put(uint64_t e, int f, uint32_t v) {
    return e | ((uint64_t)(v & FIELD_MASK) << (FIELD_BITS * f));
}
// (on the entry's 32-bit halves: the device holds them in two scalar registers)
FR_HD constexpr uint32_t get(uint64_t e, int f) {
    const uint32_t lo = (uint32_t)e, hi = (uint32_t)(e >> 32);
    const int s = FIELD_BITS * f;
    return (s + FIELD_BITS <= 32 ? lo >> s : s >= 32 ? hi >> (s - 32) : (lo >> s) | (hi << (32 - s))) & FIELD_MASK;
}
FR_HD constexpr uint32_t step(uint64_t e) { return get(e, 0); }
FR_HD constexpr uint32_t pair_i(uint64_t e, int b) { return get(e, 1 + 2 * b); }
FR_HD constexpr uint32_t pair_j(uint64_t e, int b) { return get(e, 2 + 2 * b); }
constexpr uint64_t END_ENTRY = END;

// The table's build, shared by the rotation's prologue and tools/step_sched_check.cpp.  Bit
// t % 64 of live[t / 64] is set when step t runs; a live step's entry goes to its rank among
// the live steps, the end entry to the rank of t = steps.
// set bits of live[] below bit t (word t / 64 is read only when t % 64 != 0)
FR_HD int rank_below(const uint64_t* live, int t) {
    int rank = 0;
    for (int w = 0; w < (t >> 6); ++w) rank += __builtin_popcountll(live[w]);
    const uint64_t mine = (t & 63) ? live[t >> 6] : 0;
    return rank + __builtin_popcountll(mine & ((1ULL << (t & 63)) - 1));
}
// step t's entry for B bootstraps: bootstrap b's mod-switched elements at abar + b * stride
template <int B>
FR_HD uint64_t entry_of(const uint16_t* abar, int stride, int t) {
    static_assert(1 + 2 * B <= FIELDS, "the step and B pairs in one entry");
    uint64_t e = put(0, 0, (uint32_t)t);
FR_UNROLL
    for (int b = 0; b < B; ++b) {
        e = put(e, 1 + 2 * b, abar[b * stride + 2 * t]);
        e = put(e, 2 + 2 * b, abar[b * stride + 2 * t + 1]);
    }
    return e;
}

static_assert(step(put(put(put(0, 0, 370), 1, 4095), 2, 0)) == 370 && pair_i(put(put(0, 0, 370), 1, 4095), 0) == 4095 &&
                  pair_j(put(put(put(put(0, 0, 0), 3, 4095), 4, 4095), 2, 1), 1) == 4095,
              "fields do not overlap");

}  // namespace step_sched
}  // namespace fr
