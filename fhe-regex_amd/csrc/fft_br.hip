// Blind rotation on the 2^64 torus with an f64 negacyclic FFT (FR_RING_FFT),
// gfx950.  The ring, the transform and every floating-point operation are
// specified in fft.h; oracle/tfhe_oracle.c restates the same sequence.
// (File named fft_br.hip so its object does not collide with fft.cpp.)
//
//   k_blind_rotate_fft<N,K,E,LAT,B> (and its _kp, _acc and _dual variants): modulus
//     switch, test-polynomial accumulator (u64), the unrolled blind rotation (one
//     step per pair of LWE coefficients, three GGSWs, see rns_br.hip), multi-value
//     w-step and sample extract -- outputs are already torus LWEs, no ring
//     conversion.  Every compile-time fact of a launch shape -- geometry, threads,
//     key-load schedule, LDS layout -- is a constant of FbrShape (FbrDualShape).
//   k_key_products<N>: the MAC's key-only half, ahead of the smallest launches.
//
// Geometry: one workgroup per bootstrap (pair shape: two), (K + 1) * M/E lanes (M = N/2
// complex points per polynomial, E per lane, whole waves per polynomial).  The
// log2 M transform stages run as register phases of log2 E stages joined by
// LDS exchanges of 16-B complex values (conflict-free maps of geo.h with
// 8-lane b128 groups).  Per step a lane: gadget digits of its 2E accumulator
// coefficients (local, exact), forward FFT, MAC with the three Fourier GGSWs
// (coalesced [w][r][c][m][lane] layout) and their slot-wise monomial factors
// psi^(e L) - 1 (quadrant table in LDS), inverse FFT, exact f64 -> torus
// conversion and u64 accumulate.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <cstring>

#include "device_impl.h"
#include "fft.h"
#include "geo.h"
#include "step_sched.h"

namespace fr {

template <int M, int E>
using FGeo = NttGeo<M, E, 3, fft_layout_variant(ilog2c(M), ilog2c(E))>;
template <int M, int E>
constexpr int FV = fft_layout_variant(ilog2c(M), ilog2c(E));

__device__ __forceinline__ void cfwd(double2& x, double2& y, double2 c) { fft::fwd_bf(x.x, x.y, y.x, y.y, c.x, c.y); }
__device__ __forceinline__ void cinv(double2& u, double2& v, double2 c) { fft::inv_bf(u.x, u.y, v.x, v.y, c.x, c.y); }

// k = 1 (log2 M even, E = 4): every phase is two stages s0 = 2p, s1 = 2p + 1 and the
// inverse takes them as one radix-4 group (fft.h inv_r4).  A lane's twiddles of such a
// phase are c (stage s0, both pairs), ca (stage s1, pair 0/1; pair 2/3 has i ca exactly,
// fft::Tables) and cc = c ca (inverse only).
template <int M, int E>
constexpr bool fradix4() {
    return E == 4 && FGeo<M, E>::LOG % 2 == 0;
}
template <int M, int E>
struct FTwr {
    static constexpr int COUNT = fradix4<M, E>() ? FGeo<M, E>::NPH * 3 : FGeo<M, E>::LOG * (E / 2);
    double2 v[COUNT];
};
// i c (exact: a swap and a sign)
__device__ __forceinline__ double2 fmul_i(double2 c) { return make_double2(-c.y, c.x); }
__device__ __forceinline__ void cinv_r4(double2 (&x)[4], double2 c, double2 ca, double2 cc) {
    fft::inv_r4(x[0].x, x[0].y, x[1].x, x[1].y, x[2].x, x[2].y, x[3].x, x[3].y, c.x, c.y, ca.x, ca.y, cc.x, cc.y);
}
// The radix-2 butterflies of phase p: fn(s, m, dm) for each of its stages s (REV: last
// stage first, the inverse's order) and each element m that pairs with m + dm.
template <class G, int E, int p, bool REV, class F>
__device__ __forceinline__ void for_butterflies(F&& fn) {
#pragma unroll
    for (int i = 0; i < G::s_end(p) - G::s_begin(p); ++i) {
        const int s = REV ? G::s_end(p) - 1 - i : G::s_begin(p) + i;
        const int dm = 1 << (G::LOG - 1 - s - G::lo(p));
#pragma unroll
        for (int m = 0; m < E; ++m) {
            if (m & dm) continue;
            fn(s, m, dm);
        }
    }
}
// stage s's entry of a twiddle table for element m of the lane whose layout-p base is b
template <class G, int p>
__device__ __forceinline__ double2 ftw_at(const double2* tw, int b, int s, int m) {
    return (tw + (b >> (G::LOG - s)))[(1 << s) + (G::template moff<p>(m) >> (G::LOG - s))];
}
// the radix-4 twiddles (c, ca) of phase p for this lane from the LDS table
template <int M, int E, int p>
__device__ __forceinline__ void ftw_r4(const double2* tw, int tl, double2& c, double2& ca) {
    using G = FGeo<M, E>;
    constexpr int s0 = G::s_begin(p), s1 = s0 + 1;
    const int b = G::template base<p>(tl);
    c = ftw_at<G, p>(tw, b, s0, 0);
    ca = ftw_at<G, p>(tw, b, s1, 0);
}

template <int M, int E, int p>
__device__ __forceinline__ void ffwd_phase(double2 (&x)[E], const double2* tw, int tl) {
    using G = FGeo<M, E>;
    const int b = G::template base<p>(tl);
    for_butterflies<G, E, p, false>([&](int s, int m, int dm) { cfwd(x[m], x[m + dm], ftw_at<G, p>(tw, b, s, m)); });
}
template <int M, int E, int p>
__device__ __forceinline__ void finv_phase(double2 (&x)[E], const double2* tw, int tl) {
    using G = FGeo<M, E>;
    const int b = G::template base<p>(tl);
    for_butterflies<G, E, p, true>([&](int s, int m, int dm) { cinv(x[m], x[m + dm], ftw_at<G, p>(tw, b, s, m)); });
}
// (radix-4 phases: cc = c ca from the product table twc, indexed like c)
template <int M, int E, int p>
__device__ __forceinline__ void finv_phase_lds(double2 (&x)[E], const double2* tw, const double2* twc, int tl) {
    if constexpr (fradix4<M, E>()) {
        using G = FGeo<M, E>;
        double2 c, ca;
        ftw_r4<M, E, p>(tw, tl, c, ca);
        const double2 cc = ftw_at<G, p>(twc, G::template base<p>(tl), G::s_begin(p), 0);
        cinv_r4(x, c, ca, cc);
    } else {
        finv_phase<M, E, p>(x, tw, tl);
    }
}

// Latency shape: a lane's twiddles are the same every step (they depend on the
// lane, the stage and the element only), so they are read from LDS once and
// kept in registers (FTwr): LOG * E / 2 complex values, index (s, k-th butterfly of s).
// The twiddles of phase p are wave-uniform when every lane of a wave reads the same table
// entry for each of the phase's stages (the index bits the entry depends on sit on element or
// wave bits of that layout: phases 0 and 1 of the k = 1 geometry).  Those stay in SGPRs, which
// frees 4 VGPRs per complex twiddle (pair shape: 16 of its 256, where it spilled 16).
template <int M, int E, int p>
constexpr bool ftw_wave_uniform() {
    using G = FGeo<M, E>;
    for (int w = 0; w * 64 < G::T; ++w)
        for (int s = G::s_begin(p); s < G::s_end(p); ++s) {
            const int ref = geo_base(G::LOG, G::e, p, w * 64, FV<M, E>) >> (G::LOG - s);
            for (int l = 1; l < 64; ++l)
                if ((geo_base(G::LOG, G::e, p, w * 64 + l, FV<M, E>) >> (G::LOG - s)) != ref) return false;
        }
    return true;
}
__device__ __forceinline__ double2 fwave_uniform(double2 v) {
    const unsigned long long a = (unsigned long long)__double_as_longlong(v.x);
    const unsigned long long b = (unsigned long long)__double_as_longlong(v.y);
    const unsigned a0 = __builtin_amdgcn_readfirstlane((unsigned)a), a1 = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    const unsigned b0 = __builtin_amdgcn_readfirstlane((unsigned)b), b1 = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    return make_double2(__longlong_as_double((long long)(((unsigned long long)a1 << 32) | a0)),
                        __longlong_as_double((long long)(((unsigned long long)b1 << 32) | b0)));
}
// (UNI of ftw_load_phase: the pair and dual shapes; the latency shape lost 5% to a worse schedule at
// 190 VGPRs and keeps its twiddles in VGPRs: tools/README.md, FR_TW_SGPR_PAIR)
template <int M, int E>
constexpr int ftw_index(int s, int m) {
    const int d = FGeo<M, E>::LOG - 1 - s - FGeo<M, E>::lo(s / FGeo<M, E>::e);
    return s * (E / 2) + ((m >> (d + 1)) << d) + (m & ((1 << d) - 1));
}
template <int M, int E, int p, bool UNI = false>
__device__ __forceinline__ void ftw_load_phase(FTwr<M, E>& twr, const double2* tw, int tl) {
    using G = FGeo<M, E>;
    if constexpr (fradix4<M, E>()) {
        double2 c, ca, cc;
        ftw_r4<M, E, p>(tw, tl, c, ca);
        fft::cmul(c.x, c.y, ca.x, ca.y, cc.x, cc.y);
        if constexpr (UNI && ftw_wave_uniform<M, E, p>()) {
            c = fwave_uniform(c);
            ca = fwave_uniform(ca);
            cc = fwave_uniform(cc);
        }
        twr.v[3 * p] = c, twr.v[3 * p + 1] = ca, twr.v[3 * p + 2] = cc;
        if constexpr (p + 1 < G::NPH) ftw_load_phase<M, E, p + 1, UNI>(twr, tw, tl);
        return;
    }
    const int b = G::template base<p>(tl);
    for_butterflies<G, E, p, false>([&](int s, int m, int) { twr.v[ftw_index<M, E>(s, m)] = ftw_at<G, p>(tw, b, s, m); });
    if constexpr (p + 1 < G::NPH) ftw_load_phase<M, E, p + 1, UNI>(twr, tw, tl);
}
template <int M, int E, int p>
__device__ __forceinline__ void ffwd_phase_r(double2 (&x)[E], const FTwr<M, E>& twr) {
    using G = FGeo<M, E>;
    if constexpr (fradix4<M, E>()) {  // stage s0: pairs (0, 2), (1, 3); stage s1: (0, 1), (2, 3)
        const double2 c = twr.v[3 * p], ca = twr.v[3 * p + 1];
        cfwd(x[0], x[2], c);
        cfwd(x[1], x[3], c);
        cfwd(x[0], x[1], ca);
        cfwd(x[2], x[3], fmul_i(ca));
        return;
    }
    for_butterflies<G, E, p, false>([&](int s, int m, int dm) { cfwd(x[m], x[m + dm], twr.v[ftw_index<M, E>(s, m)]); });
}
template <int M, int E, int p>
__device__ __forceinline__ void finv_phase_r(double2 (&x)[E], const FTwr<M, E>& twr) {
    using G = FGeo<M, E>;
    if constexpr (fradix4<M, E>()) {
        cinv_r4(x, twr.v[3 * p], twr.v[3 * p + 1], twr.v[3 * p + 2]);
        return;
    }
    for_butterflies<G, E, p, true>([&](int s, int m, int dm) { cinv(x[m], x[m + dm], twr.v[ftw_index<M, E>(s, m)]); });
}

// Register exchanges.  An exchange between adjacent layouts transposes the lane's
// element bits with the lane bits that carry the arriving index bits.  When element
// bit j leaves through the same lane bit k that brings in the next layout's element
// bit j, and k is 4 or 5 (row pairs / wave halves), the transpose of each pair
// (A = x[m], B = x[m | 2^j]) is one v_permlane16/32_swap per dword: lanes with bit k
// clear keep A and receive the partner's A as B; lanes with bit k set keep B and
// receive the partner's B as A.  No LDS traffic and no barrier (E = 4: the exchange
// between layouts 1 and 2 of both transforms).
template <int M, int E, int PF, int PT>
constexpr int fperm_lane_bit(int j) {
    using G = FGeo<M, E>;
    const int out = G::lo(PF) + j, in = G::lo(PT) + j;
    int kb = -1, kc = -1;
    for (int b = 0; b < 6; ++b) {
        if (G::lane_bit(PT, b) == out) kb = b;
        if (G::lane_bit(PF, b) == in) kc = b;
    }
    return kb == kc ? kb : -1;
}
template <int M, int E, int PF, int PT>
constexpr bool fperm_ok() {
    using G = FGeo<M, E>;
    if (PF == PT || (PF - PT != 1 && PT - PF != 1)) return false;
    for (int j = 0; j < G::e; ++j) {
        const int k = fperm_lane_bit<M, E, PF, PT>(j);
        if (k != 4 && k != 5) return false;
    }
    // every other lane bit carries the same index bit in both layouts
    for (int b = 0; b < 8; ++b) {
        bool swapped = false;
        for (int j = 0; j < G::e; ++j) swapped |= fperm_lane_bit<M, E, PF, PT>(j) == b;
        if (!swapped && G::lane_bit(PF, b) != G::lane_bit(PT, b)) return false;
    }
    return true;
}
template <int K>
__device__ __forceinline__ void fperm_swap(double& a, double& b) {
    static_assert(K == 4 || K == 5, "permlane swaps serve lane bits 4 and 5");
    const unsigned long long ua = (unsigned long long)__double_as_longlong(a);
    const unsigned long long ub = (unsigned long long)__double_as_longlong(b);
    unsigned lo0 = (unsigned)ua, hi0 = (unsigned)(ua >> 32), lo1 = (unsigned)ub, hi1 = (unsigned)(ub >> 32);
    if constexpr (K == 4) {
        const auto l = __builtin_amdgcn_permlane16_swap(lo0, lo1, false, false);
        const auto h = __builtin_amdgcn_permlane16_swap(hi0, hi1, false, false);
        lo0 = l[0], lo1 = l[1], hi0 = h[0], hi1 = h[1];
    } else {
        const auto l = __builtin_amdgcn_permlane32_swap(lo0, lo1, false, false);
        const auto h = __builtin_amdgcn_permlane32_swap(hi0, hi1, false, false);
        lo0 = l[0], lo1 = l[1], hi0 = h[0], hi1 = h[1];
    }
    a = __longlong_as_double((long long)(((unsigned long long)hi0 << 32) | lo0));
    b = __longlong_as_double((long long)(((unsigned long long)hi1 << 32) | lo1));
}
template <int M, int E, int PF, int PT, int j = 0>
__device__ __forceinline__ void fperm_exchange(double2 (&x)[E]) {
    constexpr int K = fperm_lane_bit<M, E, PF, PT>(j);
#pragma unroll
    for (int m = 0; m < E; ++m) {
        if (m & (1 << j)) continue;
        fperm_swap<K>(x[m].x, x[m | (1 << j)].x);
        fperm_swap<K>(x[m].y, x[m | (1 << j)].y);
    }
    if constexpr (j + 1 < FGeo<M, E>::e) fperm_exchange<M, E, PF, PT, j + 1>(x);
}

// Cross-wave exchanges that only transpose the element bits with the wave bits (lane bits
// 6, 7), position by position, with every other lane bit in place: a lane keeps the element
// whose index equals its wave bits, in the same register (forward 0 -> 1, inverse 1 -> 0 of
// k = 1), so it writes and reads E - 1 elements instead of E.  Throughput shape only (XK): the
// latency shape lost 3% to the wave-uniform branches (tools/README.md, FR_XKEEP)
template <int M, int E, int PF, int PT>
constexpr bool fxkeep_ok() {
    using G = FGeo<M, E>;
    if ((1 << (6 + G::e)) > G::T || PF == PT) return false;
    for (int b = 0; (1 << b) < G::T; ++b) {
        if (b >= 6 && b < 6 + G::e) {
            if (G::lane_bit(PF, b) != G::lo(PT) + (b - 6) || G::lane_bit(PT, b) != G::lo(PF) + (b - 6)) return false;
        } else if (G::lane_bit(PF, b) != G::lane_bit(PT, b)) {
            return false;
        }
    }
    return true;
}
// B bootstraps per workgroup (pair shape: B = 2), bootstrap b's rows at row + b BS: one
// barrier serves the exchanges of all B
template <int M, int E, int PF, int PT, bool PRE, bool XK, int B, int BS>
__device__ __forceinline__ void fexchange(double2 (&x)[B][E], double2* row, int tl) {
    using G = FGeo<M, E>;
    if constexpr (fperm_ok<M, E, PF, PT>()) {
        // a pre-barrier would also order the next exchange's writes: keep the plan's barriers
        static_assert(!PRE, "register exchanges replace only exchanges without a pre-barrier");
#pragma unroll
        for (int b = 0; b < B; ++b) fperm_exchange<M, E, PF, PT>(x[b]);
    } else {
        constexpr int X = PF < PT ? PF : PT;
        double2* rf = row + G::template at<X>(G::template base<PF>(tl));
        double2* rt = row + G::template at<X>(G::template base<PT>(tl));
        if constexpr (PRE) __syncthreads();
        if constexpr (XK && fxkeep_ok<M, E, PF, PT>()) {  // the kept element: wave-uniform branches around its store and load
            const int q = __builtin_amdgcn_readfirstlane((tl >> 6) & (E - 1));
#pragma unroll
            for (int b = 0; b < B; ++b)
#pragma unroll
                for (int m = 0; m < E; ++m)
                    if (m != q) rf[b * BS + G::template at<X>(G::template moff<PF>(m))] = x[b][m];
            __syncthreads();
#pragma unroll
            for (int b = 0; b < B; ++b)
#pragma unroll
                for (int m = 0; m < E; ++m)
                    if (m != q) x[b][m] = rt[b * BS + G::template at<X>(G::template moff<PT>(m))];
            return;
        }
#pragma unroll
        for (int b = 0; b < B; ++b)
#pragma unroll
            for (int m = 0; m < E; ++m) rf[b * BS + G::template at<X>(G::template moff<PF>(m))] = x[b][m];
        if constexpr (G::template wave_local<PF, PT>() && G::wave_top(PF)) wave_sync();
        else __syncthreads();
#pragma unroll
        for (int b = 0; b < B; ++b)
#pragma unroll
            for (int m = 0; m < E; ++m) x[b][m] = rt[b * BS + G::template at<X>(G::template moff<PT>(m))];
    }
}
// every LDS exchange conflict-free; register exchanges need no map, except that map XL
// also serves the MAC's last-layout accesses
template <int M, int E, int X = 0>
constexpr bool fexchanges_conflict_free() {
    using G = FGeo<M, E>;
    if constexpr (X + 1 >= G::NPH) return true;
    else
        return ((fperm_ok<M, E, X, X + 1>() && X != G::XL) || G::template b128_exchange_ok<X>()) &&
               fexchanges_conflict_free<M, E, X + 1>();
}
// NOPRE: the rows of the forward transform + MAC and of the inverse transform
// are separate buffers (latency shape).  Then no write needs a barrier before
// it: a transform's first cross-wave write follows the previous cross-wave
// exchange's barrier, which every wave reaches only after its last read of the
// other buffer; the inverse's first write (own slots) no longer meets the other
// polynomials' MAC reads.
// TWR: twiddles from the lane's registers (twr), else from the LDS table tw.
// hook(integral_constant<p>) runs after phase p's butterflies (before its exchange).
// CARRY: a pre-barrier owed by a register exchange (which writes no LDS) moves to the
// next LDS exchange's write.
// B, BS: B transforms side by side (rows b BS apart), their exchanges sharing barriers.
template <int M, int E, int p, bool NOPRE, bool TWR, int B, int BS, bool CARRY = false, class Hook>
__device__ __forceinline__ void fforward_from(double2 (&x)[B][E], double2* row, const FTwr<M, TWR ? E : 2>& twr,
                                              const double2* tw, int tl, Hook&& hook) {
#pragma unroll
    for (int b = 0; b < B; ++b) {
        if constexpr (TWR) ffwd_phase_r<M, E, p>(x[b], twr);
        else ffwd_phase<M, E, p>(x[b], tw, tl);
    }
    hook(std::integral_constant<int, p>{});
    if constexpr (p + 1 < FGeo<M, E>::NPH) {
        constexpr bool pre = !NOPRE && (FGeo<M, E>::template fwd_pre<p>() || CARRY), reg = fperm_ok<M, E, p, p + 1>();
        fexchange<M, E, p, p + 1, reg ? false : pre, !NOPRE, B, BS>(x, row, tl);
        fforward_from<M, E, p + 1, NOPRE, TWR, B, BS, reg && pre>(x, row, twr, tw, tl, hook);
    }
}
template <int M, int E, int p, bool NOPRE, bool TWR, int B, int BS, bool CARRY = false>
__device__ __forceinline__ void finverse_from(double2 (&x)[B][E], double2* row, const FTwr<M, TWR ? E : 2>& twr,
                                              const double2* tw, const double2* twc, int tl) {
    if constexpr (TWR && B > 1 && fradix4<M, E>()) {
        // pair shape: cc = c ca recomputed per phase (20 fewer live VGPRs; the same
        // fft::cmul as ftw_load_phase, so the same bits), shared by the B transforms
        const double2 c = twr.v[3 * p], ca = twr.v[3 * p + 1];
        double2 cc;
        fft::cmul(c.x, c.y, ca.x, ca.y, cc.x, cc.y);
#pragma unroll
        for (int b = 0; b < B; ++b) cinv_r4(x[b], c, ca, cc);
    } else {
#pragma unroll
        for (int b = 0; b < B; ++b) {
            if constexpr (TWR) finv_phase_r<M, E, p>(x[b], twr);
            else finv_phase_lds<M, E, p>(x[b], tw, twc, tl);
        }
    }
    if constexpr (p > 0) {
        constexpr bool pre = !NOPRE && (FGeo<M, E>::template inv_pre<p>() || CARRY), reg = fperm_ok<M, E, p, p - 1>();
        fexchange<M, E, p, p - 1, reg ? false : pre, !NOPRE, B, BS>(x, row, tl);
        finverse_from<M, E, p - 1, NOPRE, TWR, B, BS, reg && pre>(x, row, twr, tw, twc, tl);
    }
}

// LDS slot of psi^k in the monomial table.  A lane's lookup index is k = e L mod 2N
// with L = 1 + 4 brv(lane slot base), so the 16 lanes of a b128 read group share
// k mod 32 (every lookup one bank quad: ~13-way conflicts).  Folding bits 5..9 into
// the quad bits spreads them (1.8-way on average over e); a bijection on [0, 2^10)
// blocks, so it serves the N-entry and the N/2-entry (quadrant) table alike.
__device__ __forceinline__ int psi_slot(int k) { return k ^ ((k >> 6) & 15) ^ ((k >> 5) & 1); }

// Slot factor psi^(e (Lb + M sm)) = i^q psi^(e Lb), q = (e sm) mod 4 (fft::psi_quadrant of
// the base): for odd sm, q is odd exactly when the uniform e is, so the swap of an odd turn is
// one select per base shared by the slots sm = 1, 3, and every slot adds only a uniform sign
// (i^q b = i^(q-1) (i b), q - 1 even).  The same values as psi_quadrant; 11 VALU per factor
// over a lane's 4 slots instead of ~23 (latency step loop 602 -> 584 VALU per wave-step; one
// bootstrap 1.355 -> 1.324 ms, 2048 10.00 -> 9.83 ms: profiles/r03/ab_slot_factor.log).
// A 16-way uniform branch on (a_i, a_j) mod 4 that made every turn compile-time spilled
// 14-84 VGPRs in every shape and was dropped.
__device__ __forceinline__ void slot_factor(double br, double bi, uint32_t e, uint32_t sm, double& cr, double& ci) {
    const uint32_t q = (e * sm) & 3u;
    const bool swap = (sm & 1u) && (e & 1u);
    const double ar = swap ? -bi : br, ai = swap ? br : bi;
    const long long sg = (long long)((q >> 1) & 1u) << 63;
    cr = __longlong_as_double(__double_as_longlong(ar) ^ sg);
    ci = __longlong_as_double(__double_as_longlong(ai) ^ sg);
}
// The key-only half of the MAC, defined once: everything a step's MAC forms from the Fourier
// key and the mod-switched pair (e_i, e_j) before it touches the digits.  The MAC of every
// launch shape and k_key_products call these two functions and nothing else forms these
// values, so a product is the same operations in the same order wherever it is computed.
// (a) the slot base's factor psi^(e Lb) from the LDS table psi (filled through psi_slot):
// the whole circle (k < 2N) or the quadrant table (k < N/2) and a quarter turn
template <int N, bool PSIQ>
__device__ __forceinline__ void key_psi_base(const double2* psi, uint32_t e, uint32_t Lb, double& br, double& bi) {
    const uint32_t k = __umul24(e, Lb) & (2 * N - 1);
    if constexpr (!PSIQ) {  // psi^k, k < 2N, straight from the table
        const double2 c = psi[psi_slot((int)k)];
        br = c.x;
        bi = c.y;
    } else {
        const double2 q = psi[psi_slot((int)(k & (N / 2 - 1)))];
        fft::psi_quadrant(q.x, q.y, k >> (ilog2c(N) - 1), br, bi);
    }
}
// (b) slot sm's products from its base's factors (bre, bim)[e_i, e_j][mb] and the slot's key values
// key(g, r) (r = 0: the own row B_g[P][P], r = 1 + q: the q-th other row): c_1, c_2 by
// slot_factor, c_0 = c_1 c_2, then per row K_r = sum_g B_g[r][P] (c_g - 1), g ascending, own
// row first.  16 (K + 1) VALU per slot (k = 1: 32, against 36 for sum_g (c_g - 1) y_g)
template <int K, int NB, class KeyAt>
__device__ __forceinline__ void key_products(const double (&bre)[2][NB], const double (&bim)[2][NB], int mb, uint32_t ei,
                                             uint32_t ej, uint32_t sm, KeyAt&& key, double& kor, double& koi,
                                             double (&kxr)[K], double (&kxi)[K]) {
    double cr[3], ci[3];
#pragma unroll
    for (int h = 1; h < 3; ++h)  // uniform quarter turn
        slot_factor(bre[h - 1][mb], bim[h - 1][mb], h == 1 ? ei : ej, sm, cr[h], ci[h]);
    fft::cmul(cr[1], ci[1], cr[2], ci[2], cr[0], ci[0]);
#pragma unroll
    for (int gg = 0; gg < 3; ++gg) {
        const double c1r = cr[gg] - 1.0, c1i = ci[gg];
        const double2 Bo = key(gg, 0);
        if (gg == 0) fft::cmul(Bo.x, Bo.y, c1r, c1i, kor, koi);
        else fft::cmac(Bo.x, Bo.y, c1r, c1i, kor, koi);
#pragma unroll
        for (int q = 0; q < K; ++q) {
            const double2 Bx = key(gg, 1 + q);
            if (gg == 0) fft::cmul(Bx.x, Bx.y, c1r, c1i, kxr[q], kxi[q]);
            else fft::cmac(Bx.x, Bx.y, c1r, c1i, kxr[q], kxi[q]);
        }
    }
}
// Launch shapes (Device::br_shape picks one by batch size).  What a shape is -- its geometry,
// thread count, key-load schedule and LDS layout -- is written once, in FbrShape below:
//  * latency, LAT (E = 4; launches of at most one bootstrap per CU): one
//    workgroup per CU (k = 1: 8 waves; k = 2, N = 1024: 6 waves), 256 VGPRs; a step's
//    3 x (k+1) x E Fourier GGSW slots are held in registers, loaded by the schedule KEYS
//    (two groups a step ahead, the third at the top of the step or late in the forward
//    FFT); the whole psi^k table (k < 2N: no sign flips on lookup) and two sets of
//    exchange rows (forward + MAC / inverse: 3 barriers per step instead of 5) in LDS.
//    k = 1 keeps the lane's twiddles in registers (TWR); k = 2 reads them from LDS (the
//    36 GGSW values take the registers).
//  * latency with key products (k = 1, KP; launches of at most fft_kpre_): k_key_products forms
//    every step's K_own, K_oth on the idle CUs first; the rotation loads the 2 E products of
//    the next unskipped step right after the MAC and nothing inside a step: no key, no psi
//    table, no slot factors; 483 instructions per wave-step against 713, 148 VGPRs.
//  * pair (k = 1, B = 2; launches between the latency shape's limit and fft_pair_): the
//    latency geometry with two bootstraps per workgroup.  One set of key loads, twiddle
//    registers and barriers serves both (the two workgroups a CU would run side by side
//    in the throughput shape each load the whole key and wait at their own barriers), and
//    the two transforms give each other's exchanges independent work.  LDS: both row
//    sets per bootstrap (139 KB) + the quadrant psi table; twiddles load from global once.
//  * throughput (k = 1, E = 4: 8 waves, 128 VGPRs; E = 8: 4 waves): TP_GROUPS workgroups per
//    CU (<= 80 KB of LDS each) hide each other's barriers and loads; a slot's
//    GGSW values are loaded one slot ahead in the MAC; psi^k from the quadrant
//    table (k < N/2) + quarter turns.  k = 2, N = 1024: E = 8 is one wave per
//    polynomial (every transform exchange wave-local), three workgroups per CU.
//  * dual (k = 1, FR_FFT_DUAL=1): FbrDualShape, at its kernel.
//
// When a step's Fourier GGSW group g is loaded (FbrShape::KEYS.g[g]): a forward phase p >= 0
// (after its butterflies, before its exchange), or
constexpr int KEY_AHEAD = -1;  // a step ahead: right after the previous step's MAC, when its registers are dead
constexpr int KEY_TOP = -2;    // at the top of its own step
constexpr int KEY_NEVER = -3;  // not by group: slot by slot inside the MAC (throughput), or not at all (KP)
struct FbrKeySchedule {
    int g[3];
    // the group loaded at `when` (KEY_TOP or a forward phase), 3: none
    constexpr int group_at(int when) const {
        for (int i = 0; i < 3; ++i)
            if (g[i] == when) return i;
        return 3;
    }
    // groups 0 .. ahead() - 1 are the ones loaded a step ahead
    constexpr int ahead() const { return (g[0] == KEY_AHEAD) + (g[1] == KEY_AHEAD) + (g[2] == KEY_AHEAD); }
    // ahead groups first; every other group at a place of its own, and a forward phase that
    // exists (< nph): a load after a missing phase would be skipped and the MAC would read
    // stale key registers
    constexpr bool ok(int nph) const {
        for (int i = 0; i < 3; ++i) {
            if ((g[i] == KEY_AHEAD) != (i < ahead())) return false;
            if (g[i] != KEY_AHEAD && g[i] != KEY_NEVER && (group_at(g[i]) != i || g[i] >= nph)) return false;
        }
        return true;
    }
};

template <int N_, int K_, int E_, bool LAT_, int B_ = 1, bool KP_ = false>
struct FbrShape {
    static constexpr int N = N_, K = K_, E = E_, B = B_;  // B bootstraps per workgroup
    static constexpr bool LAT = LAT_, KP = KP_;
    static constexpr int M = N / 2;
    using G = FGeo<M, E>;
    static_assert(fexchanges_conflict_free<M, E>(), "LDS maps must make every exchange conflict-free");
    static_assert(G::base_matches_geo(), "base<p> must be the index map the LDS-map proofs reason about");
    static_assert(G::key_slot_matches_idx(), "the Fourier key's lane layout is the last-phase layout");
    static_assert(!LAT || E == 4, "the latency shape holds a step's GGSW values in registers: E = 4");
    static_assert(B == 1 || (B == 2 && LAT && K == 1 && E == 4), "pair shape: the k = 1 latency geometry");
    static_assert(!KP || (LAT && B == 1 && K == 1 && E == 4), "key products: the k = 1 latency shape");

    static constexpr int T = M / E;         // lanes per polynomial
    static constexpr int NT = (K + 1) * T;  // threads: (K + 1) polynomials of M / E lanes each
    // waves per SIMD the register allocation must allow (k = 2: 2 x 6 waves (E = 4); E = 8: the
    // one-slot-ahead loads need > 168 VGPRs)
    static constexpr int MIN_WAVES = LAT ? 2 : K == 1 ? (E == 4 ? 4 : 2) : (E == 4 ? 3 : 2);
    static constexpr int TP_GROUPS = K == 1 ? 2 : (E == 8 ? 3 : 2);  // throughput shapes: workgroups per CU
    static constexpr int NB = E >= 4 ? E / 4 : 1;                    // psi bases per lane (slots m >> 2 share one)
    static constexpr int LAST = G::NPH - 1, XL = G::XL;
    static constexpr int LOG2N2 = G::LOG + 2;        // log2(2N)
    static constexpr bool TWR = LAT && K == 1;       // twiddles in registers
    static constexpr int BS = (K + 1) * G::NP;       // one bootstrap's exchange rows
    static constexpr bool PSIQ = !LAT || B > 1;      // psi^k from the quadrant table (k < N/2) + quarter turns
    static constexpr int NPSI = KP ? 0 : PSIQ ? N / 2 : 2 * N;  // (latency shape: the whole circle, no sign flips)
    // radix-4 inverse with LDS twiddles: the product table c ca (M/2 entries, indexed like c)
    static constexpr int NTWC = fradix4<M, E>() && !TWR ? N / 4 : 0;

    // The key-load schedule.  Latency: two groups ahead; the third at the top of the step for
    // k = 1 and after forward phase 3 for k = 2.  Pair: one group ahead, the second after
    // forward phase 2 and the third after phase 4, right before the MAC barrier (the pair's 64
    // live transform values leave no room for a group across the whole transform).  The
    // measurements behind each entry: tools/README.md, "Retired switches".
    static constexpr FbrKeySchedule KEYS = !LAT || KP ? FbrKeySchedule{{KEY_NEVER, KEY_NEVER, KEY_NEVER}}
                                           : B > 1    ? FbrKeySchedule{{KEY_AHEAD, 2, 4}}
                                           : K == 1   ? FbrKeySchedule{{KEY_AHEAD, KEY_AHEAD, KEY_TOP}}
                                                      : FbrKeySchedule{{KEY_AHEAD, KEY_AHEAD, 3}};
    static constexpr int NPF = KEYS.ahead();
    static_assert(KEYS.ok(G::NPH), "key schedule: ahead groups first, then distinct places that exist");

    // The LDS layout, once: the kernel forms its pointers from these offsets and the host takes
    // BYTES.  Complex regions (offsets in double2) first, byte regions (offsets in bytes) after.
    // The pair shape (B = 2) keeps the latency shape's two row sets per bootstrap (139 KB at
    // k = 1) by dropping the forward twiddle table (its registers load from global memory once)
    // and using the quadrant psi table; its multi-value terms live in the inverse rows after the
    // loop.  (KP: no psi table)
    // The k = 1 latency shapes walk a packed step schedule (step_sched.h), built in the prologue
    // from the live-step masks; once it stands, the loop reads abar no more, so the pair shape
    // stages abar inside its inverse rows too (first written by the first step's inverse
    // transform, after the barrier that closes the build) and spends the room on the schedule.
    // (k = 2: its table of next unskipped steps, u16, in the schedule's region)
    struct Lds {
        static constexpr int XBUF = 0;  // B x (K+1) rows of NP complex: bootstrap b, row P at b BS + P NP
        static constexpr int IBUF = LAT ? XBUF + B * BS : XBUF;  // inverse-transform rows (latency shapes: separate)
        static constexpr int TW = IBUF + B * BS;                 // M forward twiddles (B = 1)
        static constexpr int PSI = TW + (B == 1 ? M : 0);        // psi^k, k < NPSI
        static constexpr int TWC = PSI + NPSI;                   // radix-4 products c ca
        static constexpr size_t LUT = 16 * (size_t)(TWC + NTWC);  // [B][16 * MAX_OUT]
        // latency shapes: bit t % 64 of live[t / 64] is set when step t runs; sched: its entries
        static constexpr size_t LIVE = LUT + B * 16 * MAX_OUT;  // [MAX_STEPS / 64] u64
        static constexpr size_t SCHED = LIVE + (LAT ? 8 * (step_sched::MAX_STEPS / 64) : 0);  // [MAX_STEPS + 1] u64
        static constexpr size_t SCHED_END = SCHED + (LAT ? 8 * (step_sched::MAX_STEPS + 1) : 0);
        static constexpr size_t ABAR = B == 1 ? SCHED_END : 16 * (size_t)IBUF;  // [B][1026] u16: n (<= 1024), zero-padded to even
        static constexpr size_t ABAR_END = ABAR + B * 2 * 1026;
        // multi-value terms [B][16 MAX_OUT] u32 and their counts [B][MAX_OUT]
        static constexpr size_t WTERMS = B == 1 ? ABAR_END : 16 * (size_t)IBUF;
        static constexpr size_t WCNT = WTERMS + 4 * B * 16 * MAX_OUT;
        static constexpr size_t WCNT_END = WCNT + 4 * B * MAX_OUT;
        static constexpr size_t BYTES = B == 1 ? WCNT_END : SCHED_END;
    };
    static_assert(B == 1 || (Lds::WCNT_END <= 16 * (size_t)(Lds::IBUF + B * BS) &&
                             Lds::ABAR_END <= 16 * (size_t)(Lds::IBUF + B * BS)),
                  "pair shape: abar (prologue) and the terms (tail) inside the inverse rows");
    static_assert(Lds::LIVE % 8 == 0 && Lds::ABAR % 4 == 0 && Lds::WTERMS % 4 == 0, "u64 / u32 regions aligned");
    static_assert(Lds::BYTES == 16 * (size_t)((LAT ? 2 : 1) * B * BS + (B == 1 ? M : 0) + NPSI + NTWC) + B * 16 * MAX_OUT +
                                    (LAT ? 8 * (step_sched::MAX_STEPS / 64 + step_sched::MAX_STEPS + 1) : 0) +
                                    (B == 1 ? 2 * 1026 + 4 * 17 * MAX_OUT : 0),
                  "LDS total: the end of the last region is the sum of the regions");
    static_assert(Lds::BYTES <= (LAT ? 160 * 1024 : 160 * 1024 / TP_GROUPS), "LDS per workgroup of the shape");
};

// Fourier-key loads: buffer loads with the key's resource in SGPRs, the uniform part
// of the offset (step, GGSW, row, slot) in soffset and the lane's byte offset as the
// only VGPR operand, so a load costs no VALU address arithmetic (gfx950 raw buffer
// resource: word 3 = 0x00020000; the key is < 2 GiB)
typedef unsigned int fr_v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t bsk_rsrc(const double2* bsk) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)bsk, 0, 0x7fffffff, 0x00020000);
}
__device__ __forceinline__ double2 bsk_load(__amdgpu_buffer_rsrc_t r, uint32_t lane_off, uint32_t uoff) {
    const fr_v4u v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)lane_off, (int)uoff, 0);
    double2 d;
    __builtin_memcpy(&d, &v, 16);
    return d;
}

// row r != P of the MAC: the q-th other polynomial in ascending order
template <int K>
__device__ __forceinline__ int other_row(int P, int q) {
    return q < P ? q : q + 1;
}
// index inside a step's key of Fourier GGSW g, row r, output column c, slot m, lane 0
// ([g][r][c][m][lane] complex values, T lanes per slot): times 16, the uniform part of a
// lane's load address
template <int K, int M, int T>
__device__ __forceinline__ constexpr uint32_t ggsw_off(int g, int r, int c, int m) {
    constexpr uint32_t GG = (uint32_t)(K + 1) * (K + 1) * M;  // complex values per Fourier GGSW
    return g * GG + (uint32_t)(r * (K + 1) + c) * M + (uint32_t)m * T;
}
// bytes of a step's three Fourier GGSWs
template <int K, int M>
constexpr uint32_t ggsw_step_bytes() {
    return 3u * 16u * (uint32_t)((K + 1) * (K + 1) * M);
}
// the 3 (K+1) Fourier GGSW values of slot m for this lane: [g][own row, other rows...]
// (row r, output column c = P; sbase: the step's byte offset)
template <int M, int T, int K>
__device__ __forceinline__ void load_slot(double2 (&B)[3][K + 1], __amdgpu_buffer_rsrc_t rs, uint32_t sbase, int P,
                                          int m, uint32_t lane_off) {
#pragma unroll
    for (int gg = 0; gg < 3; ++gg) {
        B[gg][0] = bsk_load(rs, lane_off, sbase + 16u * ggsw_off<K, M, T>(gg, P, P, m));
#pragma unroll
        for (int q = 0; q < K; ++q)
            B[gg][1 + q] = bsk_load(rs, lane_off, sbase + 16u * ggsw_off<K, M, T>(gg, other_row<K>(P, q), P, m));
    }
}
// leaf exponent mod M of the lane's slot m: L(j) = 1 + 4 brv(j) (fft::Tables::leaf, checked
// against the table in tests/test_fft.py)
template <class G>
__device__ __forceinline__ uint32_t leaf_exp(int tl, int m) {
    return (1u + 4u * (__brev((uint32_t)G::template idx<G::NPH - 1>(tl, m)) >> (32 - G::LOG))) &
           (uint32_t)((1 << G::LOG) - 1);
}
// slot m of a lane has L = Lb + M s_m with s_m = brv2(m & 3), Lb shared by the slots of equal m >> 2
__device__ __forceinline__ constexpr uint32_t brv2(int m) { return ((m & 1) << 1) | ((m >> 1) & 1); }

// value of the test polynomial at position t < N: the LUT polynomial (box N/16,
// recentred by half a box, -f(0) in the last half box) or (Delta/2) * sum X^j
template <int N>
__device__ __forceinline__ uint64_t test_poly(int t, bool direct, const uint8_t* lut0) {
    constexpr int box = N / 16, half = box / 2;
    if (!direct) return 1ULL << (DELTA_LOG - 1);
    const int mm = (t + half) / box;
    return mm < 16 ? (uint64_t)lut0[mm] << DELTA_LOG : (uint64_t)0 - ((uint64_t)lut0[0] << DELTA_LOG);
}
// sum_t d_t (X^pos_t A)[j] mod 2^64 (multi-value w-step, terms of lut_terms)
template <int N>
__device__ __forceinline__ uint64_t w_step64(const uint64_t* row, const uint32_t* terms, int nt, int j) {
    uint64_t acc = 0;
    for (int t = 0; t < nt; ++t) {
        const uint32_t tm = terms[t];
        int src = j - (int)(tm & 0xFFFF);
        int64_t d = (int64_t)(tm >> 16) - 128;
        if (src < 0) {
            src += N;
            d = -d;
        }
        acc += (uint64_t)d * row[src];
    }
    return acc;
}

// ---- the tail of a bootstrap, after the step loop, shared by k_blind_rotate_fft and
// k_blind_rotate_fft_dual (NT: threads of the workgroup, tid: this thread among them).
// The prologue (LUT / abar / bbar staging, test-polynomial accumulator) stays written out in
// both: every shared form tried changed the listing of the step loop (tools/isa_diff.py).
// Tail: one accumulator polynomial as u64 [N] at arow
template <int M, int E>
__device__ __forceinline__ void fbr_publish(uint64_t* arow, const double (&alo)[E], const double (&ahi)[E], int tl) {
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int j = FGeo<M, E>::template idx<0>(tl, m);
        arow[j] = fft::torus_of_acc(alo[m]);
        arow[j + M] = fft::torus_of_acc(ahi[m]);
    }
}
// Tail: the multi-value terms of a gate's LUTs, one thread per output
template <int N>
__device__ __forceinline__ void fbr_terms(int tid, int n_out, int kind, const uint8_t* lut, uint32_t* wterms, int* wcnt) {
    if (tid < n_out && kind == JOB_MULTI) wcnt[tid] = lut_terms<N>(lut + 16 * tid, wterms + 16 * tid);
}
// Tail: the gate's outputs from its published accumulator ab ([K+1][N]): sample extract under
// the flattened key (sign gate: +-Delta/2 + Delta/2 -> {0, Delta}), or one w-step per output
template <int N, int K, int NT>
__device__ __forceinline__ void fbr_outputs(int tid, const uint64_t* ab, const DevGate& gate, int n_out, int kind,
                                            const uint32_t* wterms, const int* wcnt, uint64_t* arena, int slot_stride) {
    constexpr int big = K * N;
    if (kind != JOB_MULTI) {
        uint64_t* out = arena + (size_t)gate.out_slot[0] * slot_stride;
        const uint64_t post = kind == JOB_SIGN ? (1ULL << (DELTA_LOG - 1)) : 0;
        for (int c = tid; c <= big; c += NT) {
            const ExtractIdx x = extract_index<N, K>(c);
            const uint64_t v = ab[x.pp * N + x.j];
            out[c] = (x.neg ? (uint64_t)0 - v : v) + (c == big ? post : 0);
        }
        return;
    }
    for (int f = 0; f < n_out; ++f) {
        const uint32_t* tf = wterms + 16 * f;
        const int nt = wcnt[f];
        uint64_t* out = arena + (size_t)gate.out_slot[f] * slot_stride;
        for (int c = tid; c <= big; c += NT) {
            const ExtractIdx x = extract_index<N, K>(c);
            const uint64_t v = w_step64<N>(ab + x.pp * N, tf, nt, x.j);
            out[c] = x.neg ? (uint64_t)0 - v : v;
        }
    }
}

// Byte sizes of the precomputed key products (k_key_products): one step's K_r values
// [P][own, other rows][m][lane] and one bootstrap's [t] of them
template <int N, int K>
constexpr uint32_t kpre_step_bytes() {
    return 16u * (uint32_t)((K + 1) * (K + 1) * (N / 2));
}

// The blind rotation of every launch shape.  KP (the latency shape, k = 1): the step's key
// products K_own, K_oth come from kpre, where k_key_products put them before this launch
// (kpre + bootstrap x steps x kpre_step_bytes), instead of the key, the psi table and the pair.
// ACC (a launch of JOB_ACC jobs only): the accumulator starts from the job's selector, a GLWE
// ciphertext [polynomial][N] of the table sel ([selector][polynomial][N] u64), every polynomial
// rotated by X^-bbar, instead of the trivial (0, .., 0, X^-bbar V(lut)).  Only the prologue
// differs: the step loop and the tail are the other variants'.
template <int N, int K, int E, bool LAT, int B, bool KP, bool ACC = false>
__device__ __forceinline__ void fbr_rotate(const uint64_t* ks, int ks_stride, int n, const DevGate* gates, int n_gates,
                                           const double2* bsk, const double2* tw_g, const double2* psi_g,
                                           const uint16_t* leaf_g, uint64_t* arena, int slot_stride, const double2* kpre,
                                           const uint64_t* sel = nullptr) {
    using S = FbrShape<N, K, E, LAT, B, KP>;
    using G = typename S::G;
    using L = typename S::Lds;
    static_assert(!(ACC && KP), "selector launches never take the key-products path");
    constexpr int M = S::M, T = S::T, NT = S::NT, NB = S::NB, BS = S::BS, LAST = S::LAST, XL = S::XL;
    constexpr int LOG2N2 = S::LOG2N2, NPSI = S::NPSI, NTWC = S::NTWC, NPF = S::NPF;
    constexpr bool TWR = S::TWR, PSIQ = S::PSIQ;
    extern __shared__ __attribute__((aligned(16))) double2 fsm[];
    uint8_t* const fsb = (uint8_t*)fsm;
    double2 *xbuf = fsm + L::XBUF, *ibuf = fsm + L::IBUF, *tw = fsm + L::TW, *psi = fsm + L::PSI, *twc = fsm + L::TWC;
    uint8_t* lut = fsb + L::LUT;
    uint16_t* abar = (uint16_t*)(fsb + L::ABAR);
    uint32_t* wterms = (uint32_t*)(fsb + L::WTERMS);
    int* wcnt = (int*)(fsb + L::WCNT);
    uint64_t* live = (uint64_t*)(fsb + L::LIVE);
    uint64_t* sched = (uint64_t*)(fsb + L::SCHED);

    const int tid = threadIdx.x;
    const int P = __builtin_amdgcn_readfirstlane(tid / T), tl = tid % T;  // wave-uniform polynomial
    // bootstrap b of this workgroup: gate B blockIdx + b (an odd count's last pair repeats its
    // gate and writes it once)
    int gb[B];
    bool has[B];
    const uint64_t* in[B];
    int n_out[B], kind[B];
#pragma unroll
    for (int b = 0; b < B; ++b) {
        const int gi = B * (int)blockIdx.x + b;
        has[b] = gi < n_gates;
        gb[b] = has[b] ? gi : B * (int)blockIdx.x;
        in[b] = ks + (size_t)gb[b] * ks_stride;
        n_out[b] = gates[gb[b]].n_out;
        kind[b] = gates[gb[b]].direct;
    }
    if constexpr (B == 1)
        for (int i = tid; i < M; i += NT) tw[i] = tw_g[i];
    for (int i = tid; i < NPSI; i += NT) psi[psi_slot(i)] = psi_g[i];
    // twc[2^s0 + b] = tw[2^s0 + b] * tw[2^(s0+1) + 2b] for even s0 (fft::cmul, as the oracle)
    for (int i = 1 + tid; i < NTWC; i += NT) {
        const int s0 = 31 - __builtin_clz((unsigned)i), b = i - (1 << s0);
        if (s0 & 1) continue;
        const double2 c = tw_g[i], ca = tw_g[(2 << s0) + 2 * b];
        fft::cmul(c.x, c.y, ca.x, ca.y, twc[i].x, twc[i].y);
    }
    uint32_t bbar[B];
#pragma unroll
    for (int b = 0; b < B; ++b) {
        uint8_t* lb = lut + b * 16 * MAX_OUT;
        uint16_t* ab = abar + b * 1026;
        for (int i = tid; i < 16 * n_out[b]; i += NT) lb[i] = gates[gb[b]].lut[i / 16][i % 16];
        for (int i = tid; i < n; i += NT) ab[i] = (uint16_t)mod_switch(in[b][i], LOG2N2);
        if (tid == 0) ab[n] = 0;  // pad an odd n
        bbar[b] = mod_switch(in[b][n], LOG2N2);
    }
    uint32_t Lb[NB];  // leaf exponents of this lane's slot bases (slots 4b)
#pragma unroll
    for (int bb = 0; bb < NB; ++bb) Lb[bb] = leaf_exp<G>(tl, 4 * bb);
    __syncthreads();

    // accumulator (f64 torus, fft.h), natural order: lane holds coefficients j and
    // j + M for j = idx<0>(tl, m); mask polynomials 0, body (polynomial K) X^-bbar * V
    double alo[B][E], ahi[B][E];
#pragma unroll
    for (int b = 0; b < B; ++b) {
        if constexpr (ACC) {
            // polynomial P of the job's selector (acc_selector: the index in the first LUT's
            // bytes), straight from global memory: 16 KB per polynomial, read once
            const uint64_t* A = sel + ((size_t)acc_selector(gates[gb[b]]) * (K + 1) + P) * N;
#pragma unroll
            for (int m = 0; m < E; ++m) {
                const int j = G::template idx<0>(tl, m);
                uint64_t v[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int s = (j + h * M + (int)bbar[b]) & (2 * N - 1);
                    const uint64_t tv = A[s & (N - 1)];
                    v[h] = s < N ? tv : (uint64_t)0 - tv;
                }
                alo[b][m] = fft::acc_of_torus(v[0]);
                ahi[b][m] = fft::acc_of_torus(v[1]);
            }
            continue;
        }
        const bool direct = kind[b] == JOB_DIRECT;
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int j = G::template idx<0>(tl, m);
            uint64_t v[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int s = (j + h * M + (int)bbar[b]) & (2 * N - 1);
                const uint64_t tv = test_poly<N>(s & (N - 1), direct, lut + b * 16 * MAX_OUT);
                v[h] = s < N ? tv : (uint64_t)0 - tv;
            }
            alo[b][m] = P == K ? fft::acc_of_torus(v[0]) : 0.0;
            ahi[b][m] = P == K ? fft::acc_of_torus(v[1]) : 0.0;
        }
    }

    double2* row = xbuf + P * G::NP;
    double2* irow = ibuf + P * G::NP;
    const int bl = G::template base<LAST>(tl);
    double2* row_bl = row + G::template at<XL>(bl);
    const double2* orow_bl[K];  // the other polynomials' rows, ascending
#pragma unroll
    for (int q = 0; q < K; ++q) orow_bl[q] = xbuf + other_row<K>(P, q) * G::NP + G::template at<XL>(bl);
    const __amdgpu_buffer_rsrc_t rs = bsk_rsrc(bsk);
    const uint32_t lane_off = 16u * (uint32_t)tl;
    const int steps = (n + 1) / 2;
    // latency shape: Fourier GGSW slots of a step for this lane, [g][own, other rows][m],
    // and (k = 1) the lane's twiddles
    // (KP: kv, the step's key products [own, other rows][m], in their place)
    double2 gv[3][K + 1][LAT && !KP ? E : 1];
    double2 kv[K + 1][KP ? E : 1];
    FTwr<M, TWR ? E : 2> twr;
    if constexpr (TWR) ftw_load_phase<M, E, 0, (B > 1)>(twr, B == 1 ? tw : tw_g, tl);  // (pair: wave-uniform ones in SGPRs)
#ifdef FR_BR_TIMING
    uint64_t tseg[6] = {0, 0, 0, 0, 0, 0};
    uint64_t tlast = __builtin_amdgcn_s_memtime();
    const uint64_t tstart = tlast;
#endif
    // latency shape: GGSW g's slots of step tt for this lane ([g][own, other rows][m])
    auto load_ggsw = [&](int gg, int tt) {
        if constexpr (!KP) {
            const uint32_t sb = (uint32_t)__builtin_amdgcn_readfirstlane(tt) * ggsw_step_bytes<K, M>();
#pragma unroll
            for (int m = 0; m < E; ++m) {
                gv[gg][0][m] = bsk_load(rs, lane_off, sb + 16u * ggsw_off<K, M, T>(gg, P, P, m));
#pragma unroll
                for (int q = 0; q < K; ++q)
                    gv[gg][1 + q][m] =
                        bsk_load(rs, lane_off, sb + 16u * ggsw_off<K, M, T>(gg, other_row<K>(P, q), P, m));
            }
        }
    };
    // KP: all of step tt's key products for this lane, 2 E loads of 1 KB per wave
    const __amdgpu_buffer_rsrc_t rk =
        bsk_rsrc(KP ? kpre + (size_t)blockIdx.x * ((size_t)((n + 1) / 2) * (kpre_step_bytes<N, K>() / 16)) : bsk);
    auto load_kp = [&](int tt) {
        if constexpr (KP) {
            const uint32_t sb = (uint32_t)__builtin_amdgcn_readfirstlane(tt) * kpre_step_bytes<N, K>();
#pragma unroll
            for (int r = 0; r <= K; ++r)
#pragma unroll
                for (int m = 0; m < E; ++m)
                    kv[r][m] = bsk_load(rk, lane_off, sb + 16u * (uint32_t)(((P * (K + 1) + r) * E + m) * T));
        }
    };
    // latency shape, LATPF: groups 0 .. NPF-1 of a step's key values (S::KEYS) are loaded one
    // step ahead -- right after the previous step's MAC, when their registers are dead --
    // so that they have the inverse FFT, the accumulate and the forward FFT to land (a
    // single CU streams ~50 GB/s of key at 3.9 us per step); the others across the
    // step's own forward FFT.  The next unskipped step comes from the schedule (no
    // control flow around the prefetch, which keeps it after the MAC's last use).
    // KP: the whole of the next unskipped step's products in that place, nothing loaded inside
    // a step.
    constexpr bool LATPF = NPF > 0;
    // The latency shapes (every one of them prefetches: LATPF or KP) walk the packed schedule
    // of step_sched.h, one entry per unskipped step: the entry of the next step is read right
    // after the MAC, where its step index addresses the prefetch, and is scalar from there on,
    // so a step starts with t, e_i and e_j in SGPRs and no LDS read in front of its digits.
    // k = 2 keeps the table of next unskipped steps (nxt, in the schedule's region) and reads
    // its pairs at the top of the step: walking the schedule, its kernel took 256 VGPRs and
    // spilled 52 bytes (profiles/step_schedule/README.md).
    constexpr bool WALK = LAT && K == 1;
    static_assert(LAT == (LATPF || KP), "every latency shape prefetches the next unskipped step");
    static_assert(!KP || WALK, "key products: addressed by the schedule's step index, first loaded after its build");
    uint16_t* nxt = (uint16_t*)sched;  // [MAX_STEPS + 2] u16 (k = 2)
    static_assert(2 * (step_sched::MAX_STEPS + 2) <= 8 * (step_sched::MAX_STEPS + 1), "nxt inside the schedule's region");
    auto sched_entry = [&](int i) {  // entry i, wave-uniform
        const uint64_t v = sched[i];
        // (the builtin returns int: through uint32_t, or the low half's bit 31 would sign-extend)
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
        return ((uint64_t)hi << 32) | lo;
    };
    // step t is skipped when every bootstrap's pair is (0, 0): X^0 acc - acc = 0.  The pair
    // shape runs a step that is zero for one bootstrap only: its factors c - 1 are exact
    // zeros, so its MAC output is 0 and the accumulate adds +-0.
    auto idle = [&](int t) {
        uint32_t z = 0;
#pragma unroll
        for (int b = 0; b < B; ++b) z |= abar[b * 1026 + 2 * t] | abar[b * 1026 + 2 * t + 1];
        return z == 0;
    };
    uint64_t ent = step_sched::END_ENTRY;  // the entry of the step at hand, then of the next one (uniform)
    int si = 0;                            // its index in the schedule
    if constexpr (WALK) {
        static_assert(NT % 64 == 0, "whole waves: a wave's ballot covers 64 consecutive steps");
        // the live steps, 64 per wave ballot (uniform trip count: every lane votes)
        for (int t0 = 0; t0 < steps; t0 += NT) {
            const int t = t0 + tid;
            const uint64_t m = __ballot(t < steps && !idle(t));
            if ((tid & 63) == 0 && t < steps) live[t >> 6] = m;
        }
        __syncthreads();
        // a live step's entry goes to its rank among the live steps; t = steps: the end entry
        for (int t = tid; t <= steps; t += NT) {
            const int rank = step_sched::rank_below(live, t);
            if (t == steps) sched[rank] = step_sched::END_ENTRY;
            else if (!idle(t)) sched[rank] = step_sched::entry_of<B>(abar, 1026, t);
        }
        __syncthreads();
        ent = sched_entry(0);
        const int t0 = (int)step_sched::step(ent);
        for (int gg = 0; gg < NPF; ++gg) load_ggsw(gg, t0 != (int)step_sched::END ? t0 : 0);
        load_kp(t0 != (int)step_sched::END ? t0 : 0);
    } else if constexpr (LATPF) {
        for (int t = tid; t <= steps; t += NT) {
            int tt = t;
            while (tt < steps && idle(tt)) ++tt;
            nxt[t] = (uint16_t)tt;
        }
        __syncthreads();
        const int t0 = __builtin_amdgcn_readfirstlane((int)nxt[0]);
        for (int gg = 0; gg < NPF; ++gg) load_ggsw(gg, t0 < steps ? t0 : 0);
    }
    // One loop for both forms (the step's body as a function of its own, called from a loop per
    // form, spilled in every shape).  WALK: the step of the entry at hand, until the end entry; the
    // post-MAC block leaves the next entry in ent.  Otherwise (k = 2 and the throughput shapes)
    // every step in turn, skipped behind a uniform branch when idle.
    auto step_from = [&](int t) { return WALK ? (int)step_sched::step(ent) : t; };
    auto more = [&](int t) { return WALK ? t != (int)step_sched::END : t < steps; };
    for (int t = step_from(0); more(t); t = step_from(t + 1)) {
        if constexpr (!WALK)
            if (idle(t)) continue;
        BR_STAMP(0);
        // the step's byte offset in the key (uniform: soffset of every load)
        const uint32_t sbase = (uint32_t)__builtin_amdgcn_readfirstlane(t) * ggsw_step_bytes<K, M>();
        // groups NPF.. of this step, where S::KEYS places them: here, or after a forward phase
        // (the group as a constant of its own: looked up in load_ggsw's argument, gv went to scratch)
        constexpr int G_TOP = S::KEYS.group_at(KEY_TOP);
        if constexpr (G_TOP < 3) {
            __builtin_amdgcn_sched_barrier(0);
            load_ggsw(G_TOP, t);
            __builtin_amdgcn_sched_barrier(0);
        }
        uint32_t ei[B], ej[B];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            if constexpr (WALK) {
                ei[b] = step_sched::pair_i(ent, b);
                ej[b] = step_sched::pair_j(ent, b);
            } else {
                ei[b] = __builtin_amdgcn_readfirstlane((uint32_t)abar[b * 1026 + 2 * t]);
                ej[b] = __builtin_amdgcn_readfirstlane((uint32_t)abar[b * 1026 + 2 * t + 1]);
            }
        }
        double bre[B][2][NB], bim[B][2][NB];
        auto psi_factors = [&]() {
#pragma unroll
            for (int b = 0; b < B; ++b)
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int bb = 0; bb < NB; ++bb)
                        key_psi_base<N, PSIQ>(psi, h == 0 ? ei[b] : ej[b], Lb[bb], bre[b][h][bb], bim[b][h][bb]);
        };
        if constexpr (LAT && B == 1 && !KP) psi_factors();
        // 1. signed gadget digits, folded: x = d_j + i d_(j+M)
        double2 x[B][E];
#pragma unroll
        for (int b = 0; b < B; ++b)
#pragma unroll
            for (int m = 0; m < E; ++m)
                x[b][m] = make_double2(fft::acc_digit<23>(alo[b][m]), fft::acc_digit<23>(ahi[b][m]));
        BR_STAMP(1);
        // 2. forward FFT (latency shapes: the key groups that S::KEYS places after a phase)
        fforward_from<M, E, 0, LAT, TWR, B, BS>(x, row, twr, tw, tl, [&](auto ph) {
            constexpr int g = S::KEYS.group_at(decltype(ph)::value);
            if constexpr (g < 3) {
                __builtin_amdgcn_sched_barrier(0);
                load_ggsw(g, t);
                __builtin_amdgcn_sched_barrier(0);
            }
        });
        BR_STAMP(2);
        // 3. MAC with the three GGSWs of the pair and their monomial factors
#pragma unroll
        for (int b = 0; b < B; ++b)
#pragma unroll
            for (int m = 0; m < E; ++m) row_bl[b * BS + G::template at<XL>(G::template moff<LAST>(m))] = x[b][m];
        // throughput shapes: slot m's GGSW values, loaded one slot ahead (E = 8) or
        // at the top of the slot (E = 4, 128 VGPRs: the other workgroup hides the wait)
        constexpr bool AHEAD = !LAT && E == 8;
        constexpr bool PRE0 = !LAT;  // slot 0 lands during the MAC barrier and row exchange
        double2 Bc[3][K + 1];
        if constexpr (PRE0) load_slot<M, T, K>(Bc, rs, sbase, P, 0, lane_off);
        __syncthreads();
        // slot factors psi^(e L) for e = a_i, a_j and their product for a_i + a_j.
        // Slot m of this lane has L = Lb + M s_m: Lb = L mod M is shared by the
        // slots of equal m >> 2 (E/4 bases per lane) and s_m = brv2(m & 3) (fft.h: L(j) =
        // 1 + 4 brv(j)).  psi^(M s e) = i^(s e) is an exact quarter turn (the table
        // itself is quadrant-reduced), so one lookup per (e, base) serves every slot.
        // latency shape: computed at the top of the step (the lookups' LDS latency hides
        // behind the digits and the forward FFT); throughput shapes: here (VGPR budget)
        if constexpr (!LAT || B > 1) psi_factors();
#pragma unroll
        for (int m = 0; m < E; ++m) {
            double2 Bn[3][K + 1];
            if constexpr (AHEAD) {
                if (m + 1 < E) load_slot<M, T, K>(Bn, rs, sbase, P, m + 1, lane_off);
                __builtin_amdgcn_sched_barrier(0);
            } else if constexpr (!LAT) {
                if (!PRE0 || m > 0) load_slot<M, T, K>(Bc, rs, sbase, P, m, lane_off);
            }
#pragma unroll
            for (int b = 0; b < B; ++b) {  // (the pair shape: both bootstraps on one set of key values)
                const double2 own = x[b][m];
                double2 oth[K];
#pragma unroll
                for (int q = 0; q < K; ++q) oth[q] = orow_bl[q][b * BS + G::template at<XL>(G::template moff<LAST>(m))];
                // per row r: K_r = sum_g B_g[r][P] (c_g - 1) (key_products, or loaded: KP); then
                // z = D_P K_P + sum_(r != P, ascending) D_r K_r  (own row first)
                double kor, koi, kxr[K], kxi[K];
                if constexpr (KP) {
                    kor = kv[0][m].x, koi = kv[0][m].y;
#pragma unroll
                    for (int q = 0; q < K; ++q) kxr[q] = kv[1 + q][m].x, kxi[q] = kv[1 + q][m].y;
                } else {
                    const uint32_t sm = brv2(m);
                    auto key_at = [&](int gg, int r) __attribute__((always_inline)) {
                        return LAT ? gv[gg][r][LAT ? m : 0] : Bc[gg][r];
                    };
                    key_products<K>(bre[b], bim[b], m >> 2, ei[b], ej[b], sm, key_at, kor, koi, kxr, kxi);
                }
                double zr, zi;
                fft::cmul(own.x, own.y, kor, koi, zr, zi);
#pragma unroll
                for (int q = 0; q < K; ++q) fft::cmac(oth[q].x, oth[q].y, kxr[q], kxi[q], zr, zi);
                x[b][m] = make_double2(zr, zi);
            }
            if constexpr (!LAT) {
                // keep the loads one slot ahead / in their slot, not all hoisted
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (AHEAD) {
#pragma unroll
                for (int gg = 0; gg < 3; ++gg)
#pragma unroll
                    for (int r = 0; r <= K; ++r) Bc[gg][r] = Bn[gg][r];
            }
        }
        if constexpr (LATPF && !WALK) {
            const int tn = __builtin_amdgcn_readfirstlane((int)nxt[t + 1]);
            __builtin_amdgcn_sched_barrier(0);
            for (int gg = 0; gg < NPF; ++gg) load_ggsw(gg, tn < steps ? tn : t);
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (WALK) {  // the next step's key, into the registers the MAC just freed
            ent = sched_entry(++si);  // (this step's pairs were last used by the MAC)
            const int tn = (int)step_sched::step(ent);
            __builtin_amdgcn_sched_barrier(0);
            for (int gg = 0; gg < NPF; ++gg) load_ggsw(gg, tn != (int)step_sched::END ? tn : t);
            load_kp(tn != (int)step_sched::END ? tn : t);
            __builtin_amdgcn_sched_barrier(0);
        }
        BR_STAMP(3);
        // 4. inverse FFT (times M; 1/M is in the key), accumulate, reduce mod 2^64
        finverse_from<M, E, LAST, LAT, TWR, B, BS>(x, irow, twr, tw, twc, tl);
        BR_STAMP(4);
#pragma unroll
        for (int b = 0; b < B; ++b)
#pragma unroll
            for (int m = 0; m < E; ++m) {
                alo[b][m] = fft::acc_reduce<23>(alo[b][m] + x[b][m].x);
                ahi[b][m] = fft::acc_reduce<23>(ahi[b][m] + x[b][m].y);
            }
        BR_STAMP(5);
    }
#ifdef FR_BR_TIMING
    if (blockIdx.x == 0 && tid == 0)
        printf("FBR_TIMING E=%d LAT=%d steps=%d total=%lu digits=%lu fwd=%lu mac=%lu inv=%lu acc=%lu top=%lu\n", E, (int)LAT,
               steps, (unsigned long)(__builtin_amdgcn_s_memtime() - tstart), (unsigned long)tseg[1],
               (unsigned long)tseg[2], (unsigned long)tseg[3], (unsigned long)tseg[4], (unsigned long)tseg[5],
               (unsigned long)tseg[0]);
#endif

    // publish the accumulator as u64 [P][N] over the exchange rows
    // (pair shape: bootstrap b's u64 rows at b (K+1) N, inside the forward rows; its terms in
    // the inverse rows)
    __syncthreads();
    uint64_t* accs = (uint64_t*)xbuf;
    static_assert(B == 1 || 8 * B * (K + 1) * N <= 16 * B * BS, "pair shape: u64 rows inside the forward rows");
#pragma unroll
    for (int b = 0; b < B; ++b) {
        fbr_publish<M, E>(accs + (b * (K + 1) + P) * N, alo[b], ahi[b], tl);
        fbr_terms<N>(tid, n_out[b], kind[b], lut + b * 16 * MAX_OUT, wterms + b * 16 * MAX_OUT, wcnt + b * MAX_OUT);
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < B; ++b)
        if (has[b])
            fbr_outputs<N, K, NT>(tid, accs + b * (K + 1) * N, gates[gb[b]], n_out[b], kind[b], wterms + b * 16 * MAX_OUT,
                                  wcnt + b * MAX_OUT, arena, slot_stride);
}

template <int N, int K, int E, bool LAT, int B = 1>
__global__ void __launch_bounds__((FbrShape<N, K, E, LAT, B>::NT), (FbrShape<N, K, E, LAT, B>::MIN_WAVES))
k_blind_rotate_fft(const uint64_t* __restrict__ ks, int ks_stride, int n, const DevGate* __restrict__ gates,
                   int n_gates, const double2* __restrict__ bsk, const double2* __restrict__ tw_g,
                   const double2* __restrict__ psi_g, const uint16_t* __restrict__ leaf_g, uint64_t* __restrict__ arena,
                   int slot_stride) {
    fbr_rotate<N, K, E, LAT, B, false>(ks, ks_stride, n, gates, n_gates, bsk, tw_g, psi_g, leaf_g, arena, slot_stride,
                                       nullptr);
}
// The key-products variant of the latency shape, after k_key_products on the same stream.  A
// kernel of its own name with the same <N, K, E, LAT, B>, so tools that read the shape off a
// kernel's template arguments (tools/pmc_summary.py) read it as a latency-shape launch.
template <int N, int K, int E, bool LAT, int B = 1>
__global__ void __launch_bounds__((FbrShape<N, K, E, LAT, B>::NT), (FbrShape<N, K, E, LAT, B>::MIN_WAVES))
k_blind_rotate_fft_kp(const uint64_t* __restrict__ ks, int ks_stride, int n, const DevGate* __restrict__ gates,
                      int n_gates, const double2* __restrict__ tw_g, uint64_t* __restrict__ arena, int slot_stride,
                      const double2* __restrict__ kpre) {
    fbr_rotate<N, K, E, LAT, B, true>(ks, ks_stride, n, gates, n_gates, nullptr, tw_g, nullptr, nullptr, arena,
                                      slot_stride, kpre);
}

// The selector variant of every shape (ACC), after the same pattern: kernels of their own name
// with the shape's <N, K, E, LAT, B>, and the selector table as one more argument.
template <int N, int K, int E, bool LAT, int B = 1>
__global__ void __launch_bounds__((FbrShape<N, K, E, LAT, B>::NT), (FbrShape<N, K, E, LAT, B>::MIN_WAVES))
k_blind_rotate_fft_acc(const uint64_t* __restrict__ ks, int ks_stride, int n, const DevGate* __restrict__ gates,
                       int n_gates, const double2* __restrict__ bsk, const double2* __restrict__ tw_g,
                       const double2* __restrict__ psi_g, const uint16_t* __restrict__ leaf_g,
                       uint64_t* __restrict__ arena, int slot_stride, const uint64_t* __restrict__ sel) {
    fbr_rotate<N, K, E, LAT, B, false, true>(ks, ks_stride, n, gates, n_gates, bsk, tw_g, psi_g, leaf_g, arena,
                                             slot_stride, nullptr, sel);
}

// Producer of the key products (k = 1, E = 4): workgroup (t, P) holds step t's three GGSW
// groups of polynomial P in registers (the lanes and loads of load_ggsw) and forms, for each
// bootstrap b of the launch with a non-idle pair, the 2 E products of every lane by
// key_psi_base and key_products -- the operations of the MAC, in its order -- and stores them
// as kpre[b][t][P][own, other][m][lane]: each store of a wave, and each later load, 1 KB
// contiguous.  The key is read once per launch whatever the batch; the steps are independent,
// so the grid fills the CUs the latency shape leaves idle.
template <int N>
__global__ void __launch_bounds__((FbrShape<N, 1, 4, true>::T))
k_key_products(const uint64_t* __restrict__ ks, int ks_stride, int n, int n_gates, const double2* __restrict__ bsk,
               const double2* __restrict__ psi_g, double2* __restrict__ kpre) {
    using S = FbrShape<N, 1, 4, true>;  // the lanes and key loads of the latency shape's polynomial
    using G = typename S::G;
    constexpr int K = S::K, E = S::E, M = S::M, T = S::T, LOG2N2 = S::LOG2N2;
    constexpr uint32_t GG = (uint32_t)(K + 1) * (K + 1) * M;  // complex values per Fourier GGSW
    __shared__ __attribute__((aligned(16))) double2 psi[N / 2];  // quadrant table psi^k, k < N/2
    const int tl = threadIdx.x, t = (int)blockIdx.x, P = (int)blockIdx.y;
    const int steps = (n + 1) / 2;
    for (int i = tl; i < N / 2; i += T) psi[psi_slot(i)] = psi_g[i];
    const __amdgpu_buffer_rsrc_t rs = bsk_rsrc(bsk);
    const uint32_t lane_off = 16u * (uint32_t)tl, sb = (uint32_t)t * ggsw_step_bytes<K, M>();
    double2 gv[3][K + 1][E];
#pragma unroll
    for (int gg = 0; gg < 3; ++gg)
#pragma unroll
        for (int m = 0; m < E; ++m) {
            // (ggsw_off, written out: through the helper this kernel's scalar address arithmetic
            // compiles to other instructions)
            gv[gg][0][m] = bsk_load(rs, lane_off, sb + 16u * (gg * GG + (uint32_t)(P * (K + 1) + P) * M + (uint32_t)m * T));
            gv[gg][1][m] = bsk_load(
                rs, lane_off, sb + 16u * (gg * GG + (uint32_t)(other_row<K>(P, 0) * (K + 1) + P) * M + (uint32_t)m * T));
        }
    const uint32_t Lb = leaf_exp<G>(tl, 0);
    __syncthreads();
    for (int b = 0; b < n_gates; ++b) {
        const uint64_t* in = ks + (size_t)b * ks_stride;
        const uint32_t ei = (uint16_t)mod_switch(in[2 * t], LOG2N2);
        const uint32_t ej = 2 * t + 1 < n ? (uint16_t)mod_switch(in[2 * t + 1], LOG2N2) : 0u;  // (an odd n: padded)
        if ((ei | ej) == 0) continue;  // an idle pair: the rotation skips the step
        double br[2][1], bi[2][1];
        key_psi_base<N, true>(psi, ei, Lb, br[0][0], bi[0][0]);
        key_psi_base<N, true>(psi, ej, Lb, br[1][0], bi[1][0]);
        double2* out = kpre + (((size_t)b * steps + t) * (K + 1) + P) * ((K + 1) * M) + tl;
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const uint32_t sm = brv2(m);
            double kor, koi, kxr[K], kxi[K];
            key_products<K>(br, bi, 0, ei, ej, sm, [&](int gg, int r) __attribute__((always_inline)) { return gv[gg][r][m]; },
                            kor, koi, kxr, kxi);
            out[m * T] = make_double2(kor, koi);
            out[(E + m) * T] = make_double2(kxr[0], kxi[0]);
        }
    }
}

// The pair shape's one instantiation is compiled in its own translation unit,
// fft_br_pair.hip, under the max-ILP machine scheduler (Makefile: PAIR_SCHED).  A/B on one box
// (profiles/r06/ab_sched.log): 512 / 2048 bootstraps 1.6% / 1.4% faster, while the latency shape
// loses 6% under that scheduler and keeps the default here.  Scheduling does not change an
// operation, so the results are the same bits.
#ifndef FR_BR_PAIR_TU
extern template __global__ void k_blind_rotate_fft<2048, 1, 4, true, 2>(const uint64_t*, int, int, const DevGate*, int,
                                                                         const double2*, const double2*, const double2*,
                                                                         const uint16_t*, uint64_t*, int);
extern template __global__ void k_blind_rotate_fft_acc<2048, 1, 4, true, 2>(const uint64_t*, int, int, const DevGate*,
                                                                             int, const double2*, const double2*,
                                                                             const double2*, const uint16_t*, uint64_t*,
                                                                             int, const uint64_t*);
#endif

// Dual shape (round 4 experiment, k = 1, FR_FFT_DUAL=1): one bootstrap per workgroup on
// M / E = 256 lanes (4 waves), each lane holding the same slots of BOTH polynomials
// (x[P][E]: the pair shape's B dimension carries the polynomial), two workgroups per CU.
// Both digit polynomials of a slot are in the lane, so the MAC needs no exchange and no
// barrier: the lane computes both output columns from all four (r, c) key values of its
// slots (the same operation sequence per output as the other shapes: bit-identical).  The
// forward and inverse share one row set (pre-barriers, as the throughput shape: 4 barriers
// per step), 54 KB of LDS per workgroup (FbrDualShape::Lds).  Each workgroup streams the whole key (the pair
// shape shares it between two bootstraps); the two workgroups of a CU have their own
// barriers, so one computes while the other waits.
template <int N_>
struct FbrDualShape {
    using C = FbrShape<N_, 1, 4, false>;  // the k = 1, E = 4 geometry: M, T, G and its proofs
    using G = typename C::G;
    static_assert(fradix4<C::M, C::E>(), "dual shape: the k = 1 geometry (radix-4 inverse)");
    static constexpr int N = N_, K = 1, E = 4, M = C::M, T = C::T, LAST = C::LAST, LOG2N2 = C::LOG2N2;
    static constexpr int B = 2;       // the polynomials of the one bootstrap
    static constexpr int NT = T;      // threads
    static constexpr int BS = G::NP;  // polynomial P's exchange row at P BS
    static constexpr int GROUPS = 2;  // workgroups per CU
    struct Lds {                      // complex regions (offsets in double2), then byte regions (in bytes)
        static constexpr int XBUF = 0;
        static constexpr int PSI = XBUF + B * BS;  // quadrant table psi^k, k < N/2
        static constexpr size_t LUT = 16 * (size_t)(PSI + N / 2);
        static constexpr size_t ABAR = LUT + 16 * MAX_OUT;
        static constexpr size_t WTERMS = ABAR + 2 * 1026;
        static constexpr size_t WCNT = WTERMS + 4 * 16 * MAX_OUT;
        static constexpr size_t BYTES = WCNT + 4 * MAX_OUT;
    };
    static_assert(Lds::BYTES == 16 * (size_t)(B * BS + N / 2) + 16 * MAX_OUT + 2 * 1026 + 4 * 17 * MAX_OUT,
                  "LDS total: the end of the last region is the sum of the regions");
    static_assert(Lds::BYTES <= 160 * 1024 / GROUPS, "dual shape: two workgroups per CU");
};
template <int N>
__global__ void __launch_bounds__((FbrDualShape<N>::NT), (FbrDualShape<N>::GROUPS))
k_blind_rotate_fft_dual(const uint64_t* __restrict__ ks, int ks_stride, int n, const DevGate* __restrict__ gates,
                        int n_gates, const double2* __restrict__ bsk, const double2* __restrict__ tw_g,
                        const double2* __restrict__ psi_g, const uint16_t* __restrict__ leaf_g,
                        uint64_t* __restrict__ arena, int slot_stride) {
    using S = FbrDualShape<N>;
    using G = typename S::G;
    using L = typename S::Lds;
    constexpr int K = S::K, E = S::E, M = S::M, B = S::B, T = S::T, NT = S::NT, LAST = S::LAST, BS = S::BS;
    constexpr int LOG2N2 = S::LOG2N2;
    extern __shared__ __attribute__((aligned(16))) double2 fsm[];
    uint8_t* const fsb = (uint8_t*)fsm;
    double2 *xbuf = fsm + L::XBUF, *psi = fsm + L::PSI;
    uint8_t* lut = fsb + L::LUT;
    uint16_t* abar = (uint16_t*)(fsb + L::ABAR);
    uint32_t* wterms = (uint32_t*)(fsb + L::WTERMS);
    int* wcnt = (int*)(fsb + L::WCNT);

    const int tl = threadIdx.x;
    const int gi = (int)blockIdx.x;
    const uint64_t* in = ks + (size_t)gi * ks_stride;
    const int n_out = gates[gi].n_out, kind = gates[gi].direct;
    for (int i = tl; i < N / 2; i += NT) psi[psi_slot(i)] = psi_g[i];
    for (int i = tl; i < 16 * n_out; i += NT) lut[i] = gates[gi].lut[i / 16][i % 16];
    for (int i = tl; i < n; i += NT) abar[i] = (uint16_t)mod_switch(in[i], LOG2N2);
    if (tl == 0) abar[n] = 0;
    const uint32_t bbar = mod_switch(in[n], LOG2N2);
    const uint32_t Lb = leaf_exp<G>(tl, 0);
    __syncthreads();

    double alo[B][E], ahi[B][E];
    {
        const bool direct = kind == JOB_DIRECT;
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int j = G::template idx<0>(tl, m);
            uint64_t v[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int s = (j + h * M + (int)bbar) & (2 * N - 1);
                const uint64_t tv = test_poly<N>(s & (N - 1), direct, lut);
                v[h] = s < N ? tv : (uint64_t)0 - tv;
            }
#pragma unroll
            for (int P = 0; P < B; ++P) {
                alo[P][m] = P == K ? fft::acc_of_torus(v[0]) : 0.0;
                ahi[P][m] = P == K ? fft::acc_of_torus(v[1]) : 0.0;
            }
        }
    }
    const __amdgpu_buffer_rsrc_t rs = bsk_rsrc(bsk);
    const uint32_t lane_off = 16u * (uint32_t)tl;
    const int steps = (n + 1) / 2;
    FTwr<M, E> twr;
    ftw_load_phase<M, E, 0, true>(twr, tw_g, tl);  // (wave-uniform twiddles in SGPRs, as the pair)
    // slot m's key values [g][r][c] (Fourier GGSW [r][c][m][lane])
    auto load_keys = [&](double2 (&Bk)[3][2][2], uint32_t sbase, int m) {
#pragma unroll
        for (int gg = 0; gg < 3; ++gg)
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c)
                    Bk[gg][r][c] = bsk_load(rs, lane_off, sbase + 16u * ggsw_off<K, M, T>(gg, r, c, m));
    };
    for (int t = 0; t < steps; ++t) {
        if ((abar[2 * t] | abar[2 * t + 1]) == 0) continue;  // (uniform) X^0 acc - acc = 0
        const uint32_t sbase = (uint32_t)__builtin_amdgcn_readfirstlane(t) * ggsw_step_bytes<K, M>();
        double2 Bc[3][2][2];
        load_keys(Bc, sbase, 0);  // slot 0 lands during the digits and the forward FFT
        const uint32_t ei = __builtin_amdgcn_readfirstlane((uint32_t)abar[2 * t]);
        const uint32_t ej = __builtin_amdgcn_readfirstlane((uint32_t)abar[2 * t + 1]);
        double2 x[B][E];
#pragma unroll
        for (int P = 0; P < B; ++P)
#pragma unroll
            for (int m = 0; m < E; ++m)
                x[P][m] = make_double2(fft::acc_digit<23>(alo[P][m]), fft::acc_digit<23>(ahi[P][m]));
        fforward_from<M, E, 0, false, true, B, BS>(x, xbuf, twr, nullptr, tl, [](auto) {});
        // slot factors (quadrant table + quarter turns, as the pair shape)
        double bre[2], bim[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t k = __umul24(h == 0 ? ei : ej, Lb) & (2 * N - 1);
            const double2 q = psi[psi_slot((int)(k & (N / 2 - 1)))];
            fft::psi_quadrant(q.x, q.y, k >> (LOG2N2 - 2), bre[h], bim[h]);
        }
#pragma unroll
        for (int m = 0; m < E; ++m) {
            double2 Bn[3][2][2];
            if (m + 1 < E) load_keys(Bn, sbase, m + 1);
            __builtin_amdgcn_sched_barrier(0);
            const uint32_t sm = brv2(m);
            double cr[3], ci[3];
#pragma unroll
            for (int h = 1; h < 3; ++h) slot_factor(bre[h - 1], bim[h - 1], h == 1 ? ei : ej, sm, cr[h], ci[h]);
            fft::cmul(cr[1], ci[1], cr[2], ci[2], cr[0], ci[0]);
            double2 z[B];
#pragma unroll
            for (int c = 0; c < B; ++c) {  // output column c: K_r = sum_g B_g[r][c] (c_g - 1), own row first
                double kor, koi, kxr, kxi;
#pragma unroll
                for (int gg = 0; gg < 3; ++gg) {
                    const double c1r = cr[gg] - 1.0, c1i = ci[gg];
                    const double2 Bo = Bc[gg][c][c], Bx = Bc[gg][1 - c][c];
                    if (gg == 0) {
                        fft::cmul(Bo.x, Bo.y, c1r, c1i, kor, koi);
                        fft::cmul(Bx.x, Bx.y, c1r, c1i, kxr, kxi);
                    } else {
                        fft::cmac(Bo.x, Bo.y, c1r, c1i, kor, koi);
                        fft::cmac(Bx.x, Bx.y, c1r, c1i, kxr, kxi);
                    }
                }
                double zr, zi;
                fft::cmul(x[c][m].x, x[c][m].y, kor, koi, zr, zi);
                fft::cmac(x[1 - c][m].x, x[1 - c][m].y, kxr, kxi, zr, zi);
                z[c] = make_double2(zr, zi);
            }
#pragma unroll
            for (int c = 0; c < B; ++c) x[c][m] = z[c];
            __builtin_amdgcn_sched_barrier(0);
            if (m + 1 < E) {
#pragma unroll
                for (int gg = 0; gg < 3; ++gg)
#pragma unroll
                    for (int r = 0; r < 2; ++r)
#pragma unroll
                        for (int c = 0; c < 2; ++c) Bc[gg][r][c] = Bn[gg][r][c];
            }
        }
        finverse_from<M, E, LAST, false, true, B, BS>(x, xbuf, twr, nullptr, nullptr, tl);
#pragma unroll
        for (int P = 0; P < B; ++P)
#pragma unroll
            for (int m = 0; m < E; ++m) {
                alo[P][m] = fft::acc_reduce<23>(alo[P][m] + x[P][m].x);
                ahi[P][m] = fft::acc_reduce<23>(ahi[P][m] + x[P][m].y);
            }
    }

    // publish the accumulator as u64 [P][N] over the rows, then sample extract / w-step
    __syncthreads();
    uint64_t* accs = (uint64_t*)xbuf;
    static_assert(8 * B * N <= 16 * B * BS, "dual shape: u64 rows inside the exchange rows");
#pragma unroll
    for (int P = 0; P < B; ++P) fbr_publish<M, E>(accs + P * N, alo[P], ahi[P], tl);
    fbr_terms<N>(tl, n_out, kind, lut, wterms, wcnt);
    __syncthreads();
    if (gi >= n_gates) return;
    fbr_outputs<N, K, NT>(tl, accs, gates[gi], n_out, kind, wterms, wcnt, arena, slot_stride);
}

#ifndef FR_BR_PAIR_TU
// ================================================================== host side
// compiled (k, N) points: the reference's PARAM_MESSAGE_2_CARRY_2 (k = 1, N = 2048) and
// BASELINE's "N = 1024" set (k = 2, N = 1024, the same 2048-bit flattened key)
// k = 1: E = 4 only (its transforms are radix-4 in the inverse, fradix4).  The one table of
// compiled shapes, for `if constexpr` and for the runtime checks alike
constexpr bool fft_supported(int K, int N, int E) {
    return (K == 1 && N == 2048 && E == 4) || (K == 2 && N == 1024 && (E == 4 || E == 8));
}

// the dynamic LDS a shape's kernel may ask for: the shape's own total
template <class S, class Kernel>
static void fft_attr(Kernel kernel) {
    HIP_CHECK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)S::Lds::BYTES));
}
template <int N, int K, int E, bool LAT, int B = 1>
static void fft_attr() {
    fft_attr<FbrShape<N, K, E, LAT, B>>(k_blind_rotate_fft<N, K, E, LAT, B>);
    fft_attr<FbrShape<N, K, E, LAT, B>>(k_blind_rotate_fft_acc<N, K, E, LAT, B>);
}

// run body(N, K) with the compile-time ring dimensions of the parameters
template <class F>
static void fft_dispatch(const Params& p, F&& body) {
    if (p.k == 1 && p.N == 2048) body(std::integral_constant<int, 2048>{}, std::integral_constant<int, 1>{});
    else if (p.k == 2 && p.N == 1024) body(std::integral_constant<int, 1024>{}, std::integral_constant<int, 2>{});
    else throw Error(FR_ERR_INVALID, "device: FFT ring needs (k, N) in {(1, 2048), (2, 1024)}");
}

void Device::init_fft() {
    if (p_.k == 2) fft_e_ = 8;  // one wave per polynomial: every transform exchange wave-local
    if (const char* ev = std::getenv("FR_FFT_LANE_ELEMS")) fft_e_ = std::atoi(ev);
    if (const char* ev = std::getenv("FR_FFT_SMALL_BATCH")) fft_small_ = (size_t)std::atol(ev);
    if (const char* ev = std::getenv("FR_FFT_PAIR_BATCH")) fft_pair_ = (size_t)std::atol(ev);
    if (const char* ev = std::getenv("FR_FFT_DUAL")) fft_dual_ = std::atoi(ev) != 0;
    if (const char* ev = std::getenv("FR_FFT_KPRE_BATCH")) fft_kpre_ = (size_t)std::atol(ev);
    if (p_.k != 1) fft_pair_ = 0, fft_kpre_ = 0;
    if (!fft_supported(p_.k, p_.N, fft_e_))
        throw Error(FR_ERR_INVALID, "device: FFT ring needs (k, N, E) in {(1, 2048, 4), (2, 1024, 4 or 8)}");
    fft_dispatch(p_, [&](auto nc, auto kc) {
        constexpr int N = decltype(nc)::value, K = decltype(kc)::value;
        fft_attr<N, K, 4, true>();
        fft_attr<N, K, 4, false>();
        if constexpr (K == 1) {
            fft_attr<N, K, 4, true, 2>();
            fft_attr<FbrShape<N, K, 4, true, 1, true>>(k_blind_rotate_fft_kp<N, K, 4, true, 1>);
            fft_attr<FbrDualShape<N>>(k_blind_rotate_fft_dual<N>);
        }
        if constexpr (fft_supported(K, N, 8)) fft_attr<N, K, 8, false>();
    });

    fft::Tables T(p_.N);
    d_ftw_.alloc(2 * (size_t)T.M);  // (complex: two doubles each)
    std::vector<fft::c64> psi(2 * (size_t)p_.N);
    for (int k = 0; k < 2 * p_.N; ++k) psi[k] = fft::psi_pow(p_.N, k);
    d_fqt_.alloc(2 * psi.size());
    d_fleaf_.alloc((size_t)T.M);
    HIP_CHECK(hipMemcpy(d_ftw_.get(), T.tw.data(), 16 * (size_t)T.M, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_fqt_.get(), psi.data(), 16 * psi.size(), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_fleaf_.get(), T.leaf.data(), 2 * (size_t)T.M, hipMemcpyHostToDevice));
}

void Device::upload_fft_bsk(const std::vector<uint64_t>& bsk) {
    const int N = p_.N, M = N / 2, kp1 = p_.k + 1;
    const size_t polys = p_.bsk_ggsw() * (size_t)kp1 * kp1;
    fft::Tables tabs(N);
    std::vector<fft::c64> four;
    fft::bsk_to_fourier(tabs, bsk, polys, four);
    // slot order -> per-lane order [poly][m][lane] (one copy per lane geometry E):
    // lane tl's element m is slot fft_key_slot(tl, m), so each load of a wave is 1 KB contiguous
    std::vector<fft::c64> lanes(four.size());
    for (int E : {8, 4}) {
        gpu::DevBuf<double>& dst = d_fbsk_[fbsk_index(E)];
        dst.reset();
        if (!fft_supported(p_.k, N, E) || !fbsk_needed(E)) continue;
        const int T = M / E, e = ilog2c(E);
        std::vector<int> slot((size_t)M);
        for (int q = 0; q < M; ++q) slot[q] = fft_key_slot(tabs.LOG, e, q % T, q / T);
        for (size_t pq = 0; pq < polys; ++pq)
            for (size_t q = 0; q < (size_t)M; ++q) lanes[pq * M + q] = four[pq * M + slot[q]];
        dst.alloc(2 * lanes.size());
        HIP_CHECK(hipMemcpy(dst.get(), lanes.data(), 16 * lanes.size(), hipMemcpyHostToDevice));
    }
}

void Device::launch_br_fft(const DevGate* d_gates, const uint64_t* d_ks, size_t n, hipStream_t s, hipEvent_t ev_start,
                           hipEvent_t ev_stop, bool acc) {
    // every blind-rotation kernel takes the same arguments; E picks the key's lane layout
    // (a selector launch: the table bound to the lane as one more)
    const uint64_t* sel = cur().sel;
    if (acc && !sel) throw Error(FR_ERR_INVALID, "selector jobs: no selector table bound");
    // (threads, LDS bytes and the key's lane layout E: the shape's own constants)
    auto launch = [&](auto shape, auto kernel, size_t grid, auto... more) {
        using S = decltype(shape);
        hipExtLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(S::NT), (uint32_t)S::Lds::BYTES, s, ev_start, ev_stop, 0,
                              d_ks, p_.ks_stride(), p_.n, d_gates, (int)n,
                              (const double2*)d_fbsk_[fbsk_index(S::E)].get(), (const double2*)d_ftw_.get(),
                              (const double2*)d_fqt_.get(), (const uint16_t*)d_fleaf_.get(), d_arena_.get(),
                              p_.slot_stride(), more...);
    };
    fft_dispatch(p_, [&](auto nc, auto kc) {
        constexpr int N = decltype(nc)::value, K = decltype(kc)::value;
        auto go = [&](auto shape) {
            using S = decltype(shape);
            const size_t grid = (n + S::B - 1) / S::B;
            if (acc) launch(shape, k_blind_rotate_fft_acc<N, K, S::E, S::LAT, S::B>, grid, sel);
            else launch(shape, k_blind_rotate_fft<N, K, S::E, S::LAT, S::B>, grid);
        };
        switch (br_shape(n, acc)) {
        case BrShape::LatencyKP:
            // the producer of the launch's key products, then the variant that loads them, in
            // stream order: the pair of kernels lies between ev_start and ev_stop, so the
            // producer's time counts as blind rotation
            if constexpr (K == 1) {
                using S = FbrShape<N, K, 4, true, 1, true>;
                const int steps = (p_.n + 1) / 2;
                const size_t per = (size_t)steps * (kpre_step_bytes<N, K>() / 8);  // doubles per bootstrap
                gpu::DevBuf<double>& kpre = cur().kpre;
                if (kpre.size() < n * per) {
                    HIP_CHECK(hipStreamSynchronize(s));  // the lane's queued rotations read the old scratch
                    kpre.alloc(n * per);
                }
                hipExtLaunchKernelGGL(k_key_products<N>, dim3((unsigned)steps, K + 1), dim3(S::T), 0, s, ev_start,
                                      nullptr, 0, d_ks, p_.ks_stride(), p_.n, (int)n,
                                      (const double2*)d_fbsk_[fbsk_index(S::E)].get(), (const double2*)d_fqt_.get(),
                                      (double2*)kpre.get());
                hipExtLaunchKernelGGL((k_blind_rotate_fft_kp<N, K, 4, true, 1>), dim3((unsigned)n), dim3(S::NT),
                                      (uint32_t)S::Lds::BYTES, s, nullptr, ev_stop, 0, d_ks, p_.ks_stride(), p_.n,
                                      d_gates, (int)n, (const double2*)d_ftw_.get(), d_arena_.get(), p_.slot_stride(),
                                      (const double2*)kpre.get());
            }
            break;
        case BrShape::Latency: go(FbrShape<N, K, 4, true>{}); break;
        case BrShape::Dual:
            if constexpr (K == 1) launch(FbrDualShape<N>{}, k_blind_rotate_fft_dual<N>, n);
            break;
        case BrShape::Pair:
            if constexpr (K == 1) go(FbrShape<N, K, 4, true, 2>{});
            break;
        case BrShape::Throughput:
            if (fft_e_ == 4) go(FbrShape<N, K, 4, false>{});
            else if constexpr (fft_supported(K, N, 8)) go(FbrShape<N, K, 8, false>{});
            break;
        }
    });
    HIP_CHECK(hipGetLastError());
}

#endif  // !FR_BR_PAIR_TU

}  // namespace fr
