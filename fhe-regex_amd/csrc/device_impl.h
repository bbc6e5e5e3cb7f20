// What the .hip translation units of the Device class share (private: device.h is the
// class's interface): the HIP error check, the stage timer, the current lane's stream, a modular inverse,
// and the device-side pieces common to the blind rotation of both rings.
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <string>

#include "device.h"

namespace fr {

#define HIP_CHECK(x)                                                                         \
    do {                                                                                     \
        hipError_t _e = (x);                                                                 \
        if (_e != hipSuccess)                                                                \
            throw Error(FR_ERR_HIP, std::string("HIP error: ") + hipGetErrorString(_e) +     \
                                        " at " __FILE__ ":" + std::to_string(__LINE__));     \
    } while (0)

// HIP-event times of K consecutive stages of one call on one stream: mark(i) opens stage i
// (and closes stage i - 1); read() follows the call's synchronisation of the stream.  Off
// (no profiling): no event is created or recorded, and read() leaves ms alone.
template <int K>
struct StageTimer {
    gpu::Event ev[K + 1];
    hipStream_t s;  // null: off
    StageTimer(bool on, hipStream_t stream) : s(on ? stream : nullptr) {
        for (int i = 0; s && i <= K; ++i) ev[i] = gpu::Event(hipEventDefault);
    }
    void mark(int i) {
        if (s) HIP_CHECK(hipEventRecord(ev[i].get(), s));
    }
    void read(double* ms) {
        for (int i = 0; s && i < K; ++i) {
            float t = 0;
            HIP_CHECK(hipEventElapsedTime(&t, ev[i].get(), ev[i + 1].get()));
            ms[i] = t;
        }
    }
};

// An install leaves a whole key or none.  Once every queued launch of every lane that reads the
// old key has finished, the guard drops it (release, then allocate: never two keys side by
// side); unless dismissed, it drops what the install has built when it goes.
template <class Drop>
struct Replacing {
    Drop drop;
    bool armed = true;
    explicit Replacing(Drop d) : drop(d) {
        HIP_CHECK(hipDeviceSynchronize());
        drop();
    }
    Replacing(const Replacing&) = delete;
    ~Replacing() {
        if (armed) drop();
    }
    void dismiss() { armed = false; }
};

// the stream of the current lane (inside Device methods)
#define STREAM (cur_stream())

// a^-1 mod a prime p < 2^32 (Fermat)
inline uint64_t mod_inverse(uint64_t a, uint64_t p) {
    uint64_t inv = 1, b = a % p, e = p - 2;
    while (e) {
        if (e & 1) inv = inv * b % p;
        b = b * b % p;
        e >>= 1;
    }
    return inv;
}

// FR_BR_TIMING (debug builds only, tools/build_variant.sh): wave 0 of workgroup 0 of a
// blind-rotation kernel accumulates s_memtime deltas of the step's segments in its
// tseg[] / tlast and prints them at the end.  The default build expands it to nothing.
#ifdef FR_BR_TIMING
#define BR_STAMP(k)                                             \
    do {                                                        \
        __builtin_amdgcn_sched_barrier(0);                      \
        const uint64_t now_ = __builtin_amdgcn_s_memtime();     \
        tseg[k] += now_ - tlast;                                \
        tlast = now_;                                           \
        __builtin_amdgcn_sched_barrier(0);                      \
    } while (0)
#else
#define BR_STAMP(k) \
    do {            \
    } while (0)
#endif

// Multi-value w-step terms of one LUT: w_f = sum_t d_t X^pos_t with
// d = f(m) - f(m-1) at m*box - box/2 and -(f(0) + f(15)) at N - box/2.
// Packed as pos | (d + 128) << 16; returns the count.
template <int N>
__device__ __forceinline__ int lut_terms(const uint8_t* lf, uint32_t* terms) {
    constexpr int box = N / 16, half = box / 2;
    int nt = 0;
    for (int tt = 1; tt <= 16; ++tt) {
        const int d = tt < 16 ? (int)lf[tt] - (int)lf[tt - 1] : -((int)lf[0] + (int)lf[15]);
        if (d != 0) terms[nt++] = (uint32_t)(tt < 16 ? tt * box - half : N - half) | ((uint32_t)(d + 128) << 16);
    }
    return nt;
}

// Sample extract under the flattened key: word c <= K N of the output LWE is coefficient j of
// accumulator polynomial pp, negated when neg (c = K N: the body, coefficient 0 of polynomial K)
struct ExtractIdx {
    int pp, j;
    bool neg;
};
template <int N, int K>
__device__ __forceinline__ ExtractIdx extract_index(int c) {
    constexpr int big = K * N;
    const int pp = c < big ? c / N : K, t = c < big ? c % N : 0;
    return {pp, t == 0 ? 0 : N - t, t != 0};
}

}  // namespace fr
