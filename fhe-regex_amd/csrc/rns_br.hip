// Blind rotation over the RNS ring (FR_RING_RNS) on MI355X (gfx950, CDNA4), and the
// Device methods that launch it.
//
//   k_blind_rotate<N,K,E>: modulus switch, test-polynomial accumulator, n CMUX
//                         steps (rotate -> gadget decompose -> forward NTT ->
//                         MAC with the NTT-domain GGSW -> inverse NTT ->
//                         accumulate), multi-value w-step, sample extract,
//                         Z_Q -> 2^64 conversion.
//   k_bsk_to_ntt<N,K,E> : one-time forward NTT of the bootstrapping key.
//   k_ring_mul<N,E>     : product of two ring elements (parity test of the NTT).
//
// Ring: Z_Q[X]/(X^N+1), Q = p0*p1 (rns.h), two 30-bit NTT primes.  One
// workgroup per bootstrap with 2*(K+1)*N/E lanes: each (polynomial, prime)
// pair is owned by N/E lanes (whole waves) holding E residues in registers.
// The log2 N NTT stages run as register-resident phases of log2 E stages
// joined by LDS exchanges.  Butterflies are Harvey-lazy with Montgomery
// products (R = 2^32): forward values stay in [0, 4p), inverse in [0, 2p),
// 32-bit adds and v_min_u32 only.  Twiddles and the BSK are in Montgomery
// form (1/N folded into the BSK); data is in normal form.  The merged-psi
// negacyclic transform: forward Cooley-Tukey with zeta[k] = psi^brv(k),
// outputs in bit-reversed slot order; inverse Gentleman-Sande with
// psi^-brv(k) = -zeta[3*2^s - 1 - k] (negation folded into the butterfly).
#include <cstdlib>
#include <type_traits>

#include "device_impl.h"
#include "geo.h"  // lane geometry and conflict-free LDS maps (shared with fft_br.hip)
#include "keys.h"
#include "rns.h"

namespace fr {

using rns::mont;
using rns::mont_lazy;
using rns::red1;
using rns::red2;

// Montgomery product a*b/2^32 in [0, 2p) (a*b < 4p^2).  (No inline asm in
// this file: the waitcnt pass drains every outstanding load before one.)
__device__ __forceinline__ uint32_t mont_lazy_d(uint32_t a, uint32_t b, uint32_t p, uint32_t pn) {
    return mont_lazy(a, b, p, pn);
}
// Montgomery reduction of a 64-bit sum of products T < 2^63: returns
// T/2^32 mod p as a value below T/2^32 + p (each use states its bound).
__device__ __forceinline__ uint32_t mont_reduce(uint64_t t, uint32_t p, uint32_t pn) {
    const uint32_t m = (uint32_t)t * pn;
    return (uint32_t)((t + (uint64_t)m * p) >> 32);
}

// Harvey-lazy Cooley-Tukey butterfly: x, y in [0, 4p) -> [0, 4p); w Montgomery
// (first = true: x already in [0, 2p), the reduction is skipped)
__device__ __forceinline__ void ct_lazy(uint32_t& x, uint32_t& y, uint32_t w, uint32_t p, uint32_t pn, bool first = false) {
    if (!first) x = red2(x, p);
    const uint32_t t = mont_lazy_d(y, w, p, pn);  // [0, 2p)
    y = x - t + 2 * p;
    x = x + t;
}
// Gentleman-Sande with the flipped twiddle w = -psi^-brv(k):
// (u, v) -> (u + v, (v - u) * w), values in [0, 2p)
__device__ __forceinline__ void gs_lazy(uint32_t& u, uint32_t& v, uint32_t w, uint32_t p, uint32_t pn) {
    const uint32_t s = red2(u + v, p);
    const uint32_t d = v - u + 2 * p;  // (0, 4p)
    v = mont_lazy_d(d, w, p, pn);
    u = s;
}

template <int N, int E, int p>
__device__ __forceinline__ void fwd_phase(uint32_t (&x)[E], const uint32_t* zt, int tl, uint32_t pm, uint32_t pn) {
    using G = NttGeo<N, E>;
    const int b = G::template base<p>(tl);
#pragma unroll
    for (int s = G::s_begin(p); s < G::s_end(p); ++s) {
        const int dm = 1 << (G::LOG - 1 - s - G::lo(p));
        const uint32_t* zs = zt + (b >> (G::LOG - s));
#pragma unroll
        for (int m = 0; m < E; ++m) {
            if (m & dm) continue;
            ct_lazy(x[m], x[m + dm], zs[(1 << s) + (G::template moff<p>(m) >> (G::LOG - s))], pm, pn, s == 0);
        }
    }
}
template <int N, int E, int p>
__device__ __forceinline__ void inv_phase(uint32_t (&x)[E], const uint32_t* zt, int tl, uint32_t pm, uint32_t pn) {
    using G = NttGeo<N, E>;
    const int b = G::template base<p>(tl);
#pragma unroll
    for (int s = G::s_end(p) - 1; s >= G::s_begin(p); --s) {
        const int dm = 1 << (G::LOG - 1 - s - G::lo(p));
        // zt[3*2^s - 1 - k], k = 2^s + (j >> (LOG-s))
        const uint32_t* zs = zt - (b >> (G::LOG - s));
#pragma unroll
        for (int m = 0; m < E; ++m) {
            if (m & dm) continue;
            gs_lazy(x[m], x[m + dm], zs[2 * (1 << s) - 1 - (G::template moff<p>(m) >> (G::LOG - s))], pm, pn);
        }
    }
}
// LDS exchange between the layouts of phases PF and PT (row = this lane's
// polynomial).  PRE: a barrier before writing (other waves may still read
// these slots); the barrier after writing is dropped for wave-local exchanges
// (the exchange and barrier plan: NttGeo, geo.h).
template <int N, int E, int PF, int PT, bool PRE = true>
__device__ __forceinline__ void exchange(uint32_t (&x)[E], uint32_t* row, int tl) {
    using G = NttGeo<N, E>;
    constexpr int X = PF < PT ? PF : PT;
    uint32_t* rf = row + G::template at<X>(G::template base<PF>(tl));
    uint32_t* rt = row + G::template at<X>(G::template base<PT>(tl));
    if constexpr (PRE) __syncthreads();
#pragma unroll
    for (int m = 0; m < E; ++m) rf[G::template at<X>(G::template moff<PF>(m))] = x[m];
    if constexpr (G::template wave_local<PF, PT>() && G::wave_top(PF)) wave_sync();
    else __syncthreads();
#pragma unroll
    for (int m = 0; m < E; ++m) x[m] = rt[G::template at<X>(G::template moff<PT>(m))];
}

template <int N, int E, int X = 0>
constexpr bool exchanges_conflict_free() {
    using G = NttGeo<N, E>;
    if constexpr (X + 1 >= G::NPH) return true;
    else return G::template banks_distinct<X>(X) && G::template banks_distinct<X>(X + 1) &&
                exchanges_conflict_free<N, E, X + 1>();
}

template <int N, int E, int p>
__device__ __forceinline__ void forward_from(uint32_t (&x)[E], uint32_t* row, const uint32_t* zt, int tl, uint32_t pm,
                                             uint32_t pn) {
    fwd_phase<N, E, p>(x, zt, tl, pm, pn);
    if constexpr (p + 1 < NttGeo<N, E>::NPH) {
        exchange<N, E, p, p + 1, NttGeo<N, E>::template fwd_pre<p>()>(x, row, tl);
        forward_from<N, E, p + 1>(x, row, zt, tl, pm, pn);
    }
}
template <int N, int E, int p>
__device__ __forceinline__ void inverse_from(uint32_t (&x)[E], uint32_t* row, const uint32_t* zt, int tl, uint32_t pm,
                                             uint32_t pn) {
    inv_phase<N, E, p>(x, zt, tl, pm, pn);
    if constexpr (p > 0) {
        exchange<N, E, p, p - 1, NttGeo<N, E>::template inv_pre<p>()>(x, row, tl);
        inverse_from<N, E, p - 1>(x, row, zt, tl, pm, pn);
    }
}
// natural order (phase-0 layout), values < 2p -> bit-reversed slots (last-phase layout), < 4p
template <int N, int E>
__device__ __forceinline__ void forward_ntt(uint32_t (&x)[E], uint32_t* row, const uint32_t* zt, int tl, uint32_t pm,
                                            uint32_t pn) {
    forward_from<N, E, 0>(x, row, zt, tl, pm, pn);
}
// last-phase layout, values < 2p -> natural order, < 2p; without the 1/N factor
template <int N, int E>
__device__ __forceinline__ void inverse_ntt(uint32_t (&x)[E], uint32_t* row, const uint32_t* zt, int tl, uint32_t pm,
                                            uint32_t pn) {
    inverse_from<N, E, NttGeo<N, E>::NPH - 1>(x, row, zt, tl, pm, pn);
}

// ------------------------------------------------------------ blind rotation
template <int N, int K, int E>
constexpr int br_threads() {
    return 2 * (K + 1) * (N / E);
}
// bootstrapping-key unrolling factor (Params::bsk_unroll): pairs for k = 1
template <int K>
constexpr int br_unroll() {
    return K == 1 ? 2 : 1;
}
template <int N, int K, int E>
constexpr size_t br_smem_bytes() {
    return sizeof(uint32_t) * (2 * (size_t)(K + 1) * NttGeo<N, E>::NP + 2 * (size_t)N) + 16 * MAX_OUT + 2 * 1026 +
           4 * 17 * MAX_OUT + (br_unroll<K>() == 2 ? sizeof(uint32_t) * 4 * (size_t)N : 0);
}
constexpr int brv_c(int x, int bits) { return bits == 0 ? 0 : ((x & 1) << (bits - 1)) | brv_c(x >> 1, bits - 1); }
// LDS position of monomial-table entry e (bank swizzle, a permutation within 32-word rows)
__device__ __forceinline__ uint32_t mono_pos(uint32_t e) { return e ^ ((e >> 5) & 31); }

// BSK NTT-domain layout [i][r][c][prime][slot]: natural (bit-reversed) slot
// order, the same for every lane geometry E, so E can be chosen per launch.
template <int N, int E>
__device__ __forceinline__ int bsk_pos(int tl, int m) {
    return NttGeo<N, E>::template idx<NttGeo<N, E>::NPH - 1>(tl, m);
}

// minimum waves per SIMD (register cap 512 / w): 4 -> 128 VGPRs, E = 8 and E = 16 alike
constexpr int BR_MIN_WAVES = 4;

// residue of sum_t d_t (X^pos_t A)[j] mod p from one residue row of A
template <class G>
__device__ __forceinline__ uint32_t w_step(const uint32_t* row, const uint32_t* terms, int nt, int j, uint32_t pm,
                                           int q) {
    constexpr int N = 1 << G::LOG;
    int64_t acc = 0;
    for (int t = 0; t < nt; ++t) {  // nt uniform, terms broadcast from LDS
        const uint32_t tm = terms[t];
        int src = j - (int)(tm & 0xFFFF);
        int d = (int)(tm >> 16) - 128;
        if (src < 0) {
            src += N;
            d = -d;
        }
        acc += (int64_t)d * (int64_t)row[G::template at<0>(src)];
    }
    // |acc| < 16 * 30 * p: shift by 512p before reducing
    return rns::reduce64((uint64_t)(acc + 512LL * pm), q);
}

// Signed gadget digits of the accumulator, split between the two prime lanes
// of each coefficient: the prime-Q lane decomposes elements [Q*E/2, (Q+1)*E/2)
// from both residues, so each digit is computed once.  Round 1 hands the
// sibling the residues it needs, round 2 the digits it did not compute (both in
// this lane's own row, at disjoint slots).  The caller's next write of the row
// (the forward NTT's first exchange) is preceded by a barrier.
template <int N, int E, int Q>
__device__ __forceinline__ void split_digits(uint32_t (&x)[E], const uint32_t (&acc)[E], uint32_t* row_b0,
                                             const uint32_t* sib_b0, uint32_t pm) {
    using G = NttGeo<N, E>;
    constexpr int HE = E / 2, M0 = Q * HE, O0 = (1 - Q) * HE;
#pragma unroll
    for (int h = 0; h < HE; ++h) row_b0[G::template at<0>(G::template moff<0>(O0 + h))] = acc[O0 + h];
    __syncthreads();
#pragma unroll
    for (int h = 0; h < HE; ++h) {
        const int off = G::template at<0>(G::template moff<0>(M0 + h));
        const uint32_t o = sib_b0[off];
        const int32_t dg = Q ? rns::decompose(o, acc[M0 + h]) : rns::decompose(acc[M0 + h], o);
        row_b0[off] = (uint32_t)dg;
        x[M0 + h] = dg >= 0 ? (uint32_t)dg : (uint32_t)(dg + (int32_t)pm);
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < HE; ++h) {
        const int32_t dg = (int32_t)sib_b0[G::template at<0>(G::template moff<0>(O0 + h))];
        x[O0 + h] = dg >= 0 ? (uint32_t)dg : (uint32_t)(dg + (int32_t)pm);
    }
}

template <int N, int K, int E>
__global__ void __launch_bounds__(2 * (K + 1) * (N / E), BR_MIN_WAVES)
k_blind_rotate(const uint64_t* __restrict__ ks, int ks_stride, int n, const DevGate* __restrict__ gates,
               const uint32_t* __restrict__ bsk, const uint32_t* __restrict__ tw, uint64_t* __restrict__ arena,
               int slot_stride) {
    using G = NttGeo<N, E>;
    static_assert(exchanges_conflict_free<N, E>(), "LDS maps must make every exchange conflict-free");
    static_assert(G::base_matches_geo(), "base<p> must be the index map the LDS-map proofs reason about");
    constexpr int NT = br_threads<N, K, E>();
    constexpr int LAST = G::NPH - 1;
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    uint32_t* xbuf = smem;                                // 2(K+1) rows of NP: row (P, q) at (2P + q) * NP
    uint32_t* zt_all = xbuf + 2 * (K + 1) * G::NP;       // 2 x N Montgomery twiddles
    uint8_t* lut = (uint8_t*)(zt_all + 2 * N);           // 16 * n_out
    uint16_t* abar = (uint16_t*)(lut + 16 * MAX_OUT);    // n (<= 1024), zero-padded to even
    uint32_t* wterms = (uint32_t*)(abar + 1026);          // multi-value terms, 16 per output
    int* wcnt = (int*)(wterms + 16 * MAX_OUT);
    uint32_t* mono = (uint32_t*)(wcnt + MAX_OUT);         // unrolled: (psi^e - 1) * R per prime, e < 2N
    constexpr int U = br_unroll<K>();

    const int tid = threadIdx.x;
    const int PQ = __builtin_amdgcn_readfirstlane(tid / G::T), tl = tid % G::T;  // wave-uniform
    const int P = PQ >> 1, q = PQ & 1;
    const uint32_t pm = rns::prime(q), pn = rns::pneg(q);
    const int g = blockIdx.x;
    const uint64_t* in = ks + (size_t)g * ks_stride;

    const int n_out = gates[g].n_out;
    const int kind = gates[g].direct;
    const bool direct = kind == JOB_DIRECT;
    for (int i = tid; i < 2 * N; i += NT) zt_all[i] = tw[i];
    for (int i = tid; i < 16 * n_out; i += NT) lut[i] = gates[g].lut[i / 16][i % 16];
    for (int i = tid; i < n; i += NT) abar[i] = (uint16_t)mod_switch(in[i], G::LOG + 1);
    if (tid == 0) abar[n] = 0;  // pad an odd n
    const uint32_t bbar = mod_switch(in[n], G::LOG + 1);
    if constexpr (U == 2) {
        __syncthreads();  // twiddles loaded
        // X^e in the NTT domain is psi^(e(2 brv(slot) + 1)); psi^e = +-zeta[brv(e mod N)]
        for (int i = tid; i < 4 * N; i += NT) {
            const int qq = i / (2 * N), e = i % (2 * N);
            const uint32_t pq = rns::prime(qq);
            const uint32_t z = zt_all[qq * N + (int)(__brev((uint32_t)(e & (N - 1))) >> (32 - G::LOG))];
            const uint32_t v = e < N ? z : rns::negm(z, pq);
            // (psi^e - 1) * 2^32 mod p, stored XOR-swizzled (mono_pos): within a
            // 32-lane half the lookups are 16 e brv5(l) + c, i.e. two banks; the
            // swizzle spreads them (22.7-way -> 1.95-way average conflict).
            mono[qq * 2 * N + mono_pos(e)] = rns::subm(v, (uint32_t)((1ULL << 32) % pq), pq);
        }
    }
    __syncthreads();
    const uint32_t* zt = zt_all + q * N;

    uint32_t* row = xbuf + PQ * G::NP;
    const uint32_t* row0 = xbuf + (2 * P) * G::NP;  // this polynomial, prime 0
    const uint32_t* row1 = row0 + G::NP;            // ... prime 1
    const int b0 = G::template base<0>(tl), bl = G::template base<LAST>(tl);
    constexpr int XL = G::XL;
    uint32_t* row_b0 = row + G::template at<0>(b0);
    const uint32_t* row0_b0 = row0 + G::template at<0>(b0);
    const uint32_t* row1_b0 = row1 + G::template at<0>(b0);
    uint32_t* row_bl = row + G::template at<XL>(bl);
    const uint32_t* xbuf_q_bl = xbuf + q * G::NP + G::template at<XL>(bl);
    uint32_t acc[E];  // canonical residues, natural order: coefficient idx<0>(tl, m)
    {
        // acc = (0, X^-bbar * V): V's residues into the body rows, then rotate
        constexpr int box = N / 16, half = box / 2;
        if (P == K) {
            const uint32_t dqr = q ? rns::DQR1 : rns::DQR0;
            const uint32_t hq = q ? rns::HQ1 : rns::HQ0;
            for (int jj = tl; jj < N; jj += G::T) {
                uint32_t v = hq;  // multi-value / sign test polynomial (Delta/2) * u
                if (direct) {
                    const int mm = (jj + half) / box;
                    v = mm < 16 ? mont(lut[mm], dqr, pm, pn) : rns::negm(mont(lut[0], dqr, pm, pn), pm);
                }
                row[G::template at<0>(jj)] = v;
            }
        }
        __syncthreads();
        const bool body = P == K;  // mask rows start at zero
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int s = (b0 + G::template moff<0>(m) + (int)bbar) & (2 * N - 1);
            const uint32_t v = row[G::template at<0>(s & (N - 1))];
            acc[m] = body ? (s < N ? v : rns::negm(v, pm)) : 0u;
        }
        __syncthreads();  // the rotated reads above touch slots other waves write next
    }

    const size_t ggsw = (size_t)(K + 1) * (K + 1) * 2 * N;
    if constexpr (U == 1) {
    for (int i = 0; i < n; ++i) {
        const int a = abar[i];
        if (a == 0) continue;  // X^0*acc - acc = 0: exact no-op (uniform branch)
        // 0. prefetch this lane's GGSW_i slots; they land during steps 1-2
        //    (__syncthreads only drains LDS counters, not these loads)
        uint32_t gv[K + 1][E];
        {
            const uint32_t* gi = bsk + (size_t)i * ggsw + (size_t)(P * 2 + q) * N + bl;
#pragma unroll
            for (int r = 0; r <= K; ++r)
#pragma unroll
                for (int m = 0; m < E; ++m) gv[r][m] = gi[(size_t)r * (K + 1) * 2 * N + G::template moff<LAST>(m)];
        }
        // 1. (X^a - 1) * acc, CRT of the two residues, signed gadget digit
        uint32_t x[E];
        // (no barrier before the write: the last inverse exchange left these
        // slots read by this wave only)
#pragma unroll
        for (int m = 0; m < E; ++m) row_b0[G::template at<0>(G::template moff<0>(m))] = acc[m];
        __syncthreads();
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int j = b0 + G::template moff<0>(m);
            const int s = (j - a) & (2 * N - 1);
            const int sp = G::template at<0>(s < N ? s : s - N);
            uint32_t v0 = row0[sp], v1 = row1[sp];
            if (s >= N) {
                v0 = rns::negm(v0, rns::P0);
                v1 = rns::negm(v1, rns::P1);
            }
            const int jo = G::template at<0>(G::template moff<0>(m));
            const int32_t dg = rns::decompose(rns::subm(v0, row0_b0[jo], rns::P0), rns::subm(v1, row1_b0[jo], rns::P1));
            x[m] = dg >= 0 ? (uint32_t)dg : (uint32_t)(dg + (int32_t)pm);
        }
        // 2. forward NTT of this lane group's digit residues
        forward_ntt<N, E>(x, row, zt, tl, pm, pn);
        // 3. external product MAC (in place): x_(P,q) = sum_r D_(r,q) * GGSW_i[r][P][q]
        //    (no barrier before the write: these slots were last read by this wave)
#pragma unroll
        for (int m = 0; m < E; ++m) row_bl[G::template at<XL>(G::template moff<LAST>(m))] = x[m];
        __syncthreads();
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int po = G::template at<XL>(G::template moff<LAST>(m));
            // sum_r D_r B_r in 64 bits (< 3 * 4p * p = 12p^2, and p < 0.235 * 2^32):
            // one reduction to [0, 3.9p), one conditional subtraction to [0, 2p)
            uint64_t ss = 0;
#pragma unroll
            for (int r = 0; r <= K; ++r) {
                const uint32_t d = (r == P) ? x[m] : xbuf_q_bl[2 * r * G::NP + po];
                ss += (uint64_t)d * gv[r][m];
            }
            x[m] = red2(mont_reduce(ss, pm, pn), pm);
        }
        // 4. inverse NTT and accumulate (1/N is folded into the BSK)
        inverse_ntt<N, E>(x, row, zt, tl, pm, pn);
#pragma unroll
        for (int m = 0; m < E; ++m) acc[m] = red1(red1(x[m], pm) + acc[m], pm);
    }
    } else {
    // Unrolled blind rotation: one step per pair (i, j) = (2t, 2t+1),
    //   acc += sum_g (X^e_g - 1) * (GGSW_3t+g [x] acc),  e = (a_i + a_j, a_i, a_j),
    // with one decomposition of acc, one forward NTT per polynomial, the three
    // monomial factors applied slot-wise in the NTT domain, one inverse NTT.
    const uint32_t* sib_b0 = xbuf + (2 * P + (1 - q)) * G::NP + G::template at<0>(b0);  // other prime, same polynomial
    const uint32_t* mono_q = mono + q * 2 * N;
    const uint32_t B0 = 2 * (__brev((uint32_t)bl) >> (32 - G::LOG)) + 1;  // slot bl + moff: 2 brv + 1 = B0 + c_m
    const int steps = (n + 1) / 2;
#ifdef FR_BR_TIMING
    uint64_t tseg[7] = {0, 0, 0, 0, 0, 0, 0};
    uint64_t tlast = __builtin_amdgcn_s_memtime();
    const uint64_t tstart = tlast;
#endif
    for (int t = 0; t < steps; ++t) {
        const uint32_t ai = abar[2 * t], aj = abar[2 * t + 1];
        if ((ai | aj) == 0) continue;  // X^0*acc - acc = 0 (uniform branch)
        BR_STAMP(0);
        // 0. prefetch the three GGSWs of this pair
        uint32_t gv[3][K + 1][E];
        {
            const uint32_t* gi = bsk + (size_t)(3 * t) * ggsw + (size_t)(P * 2 + q) * N + bl;
#pragma unroll
            for (int gg = 0; gg < 3; ++gg)
#pragma unroll
                for (int r = 0; r <= K; ++r)
#pragma unroll
                    for (int m = 0; m < E; ++m)
                        gv[gg][r][m] = gi[(size_t)gg * ggsw + (size_t)r * (K + 1) * 2 * N + G::template moff<LAST>(m)];
        }
        // 1. signed gadget digits of acc, split between the two prime lanes of a
        //    coefficient (residues and digits swapped through LDS)
        uint32_t x[E];
        if (q == 0) split_digits<N, E, 0>(x, acc, row_b0, sib_b0, pm);
        else split_digits<N, E, 1>(x, acc, row_b0, sib_b0, pm);
        BR_STAMP(1);
        // 2. forward NTT (its first exchange waits for the sibling reads above)
        forward_ntt<N, E>(x, row, zt, tl, pm, pn);
        BR_STAMP(2);
        // 3. MAC with the three GGSWs and their monomial factors
#pragma unroll
        for (int m = 0; m < E; ++m) row_bl[G::template at<XL>(G::template moff<LAST>(m))] = x[m];
        __syncthreads();
        BR_STAMP(6);
        const uint32_t e[3] = {(ai + aj) & (2 * N - 1), ai, aj};
        uint32_t eb[3];
#pragma unroll
        for (int gg = 0; gg < 3; ++gg) eb[gg] = __builtin_amdgcn_readfirstlane(e[gg]) * B0;
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int po = G::template at<XL>(G::template moff<LAST>(m));
            uint32_t d[K + 1];
#pragma unroll
            for (int r = 0; r <= K; ++r) d[r] = (r == P) ? x[m] : xbuf_q_bl[2 * r * G::NP + po];
            // y_g = sum_r D_r B_gr as one 64-bit sum (d < 4p, B < p: < 8p^2; with
            // p < 0.235 * 2^32 one reduction lands in [0, 2.87p)); then
            // z = sum_g y_g (psi^e_g - 1) < 8.6p^2 < 2^63, one reduction to
            // [0, 3p) and one subtraction of 2p: [0, 2p).
            uint64_t zs = 0;
#pragma unroll
            for (int gg = 0; gg < 3; ++gg) {
                uint64_t ys = 0;
#pragma unroll
                for (int r = 0; r <= K; ++r) ys += (uint64_t)d[r] * gv[gg][r][m];
                const uint32_t y = mont_reduce(ys, pm, pn);  // [0, 2.87p)
                const uint32_t ex = (eb[gg] + e[gg] * (uint32_t)(2 * brv_c(G::template moff<LAST>(m), G::LOG))) & (2 * N - 1);
                zs += (uint64_t)y * mono_q[mono_pos(ex)];
            }
            x[m] = red1(mont_reduce(zs, pm, pn), 2 * pm);  // [0, 3p) -> [0, 2p)
        }
        BR_STAMP(3);
        // 4. inverse NTT and accumulate (1/N is folded into the BSK)
        inverse_ntt<N, E>(x, row, zt, tl, pm, pn);
        BR_STAMP(4);
#pragma unroll
        for (int m = 0; m < E; ++m) acc[m] = red1(red1(x[m], pm) + acc[m], pm);
        BR_STAMP(5);
    }
#ifdef FR_BR_TIMING
    if (blockIdx.x == 0 && tid == 0)
        printf("BR_TIMING E=%d steps=%d total=%lu decomp=%lu fwd=%lu mac_wait=%lu mac=%lu inv=%lu acc=%lu top=%lu\n", E,
               steps, (unsigned long)(__builtin_amdgcn_s_memtime() - tstart), (unsigned long)tseg[1],
               (unsigned long)tseg[2], (unsigned long)tseg[6], (unsigned long)tseg[3], (unsigned long)tseg[4],
               (unsigned long)tseg[5], (unsigned long)tseg[0]);
#endif
    }

    // publish the accumulator: the outputs need both residues of a coefficient
    __syncthreads();
#pragma unroll
    for (int m = 0; m < E; ++m) row_b0[G::template at<0>(G::template moff<0>(m))] = acc[m];
    __syncthreads();
    const int big = K * N;
    if (kind != JOB_MULTI) {
        // sample extract (coefficient 0) under the flattened key, then Z_Q -> 2^64
        uint64_t* out = arena + (size_t)gates[g].out_slot[0] * slot_stride;
        // sign gate: +-Delta/2 (+ Delta/2) -> {0, Delta}
        const uint64_t post = kind == JOB_SIGN ? (1ULL << (DELTA_LOG - 1)) : 0;
        for (int c = tid; c <= big; c += NT) {
            // (extract_index of device_impl.h, written out: calling it changes the listing inside the step loop's span)
            const int pp = c < big ? c / N : K, t = c < big ? c % N : 0;
            const int j = t == 0 ? 0 : N - t;
            const uint32_t* r0 = xbuf + 2 * pp * G::NP;
            const int aj = G::template at<0>(j);
            uint32_t v0 = r0[aj], v1 = r0[G::NP + aj];
            if (t != 0) {
                v0 = rns::negm(v0, rns::P0);
                v1 = rns::negm(v1, rns::P1);
            }
            out[c] = rns::to_torus(v0, v1) + (c == big ? post : 0);
        }
        return;
    }
    // multi-value: acc_f = w_f * acc with w_f = sum_t d_t X^{pos_t} (small d_t)
    if (tid < n_out) wcnt[tid] = lut_terms<N>(lut + 16 * tid, wterms + 16 * tid);
    __syncthreads();
    for (int f = 0; f < n_out; ++f) {
        const uint32_t* tf = wterms + 16 * f;
        const int nt = wcnt[f];
        uint64_t* out = arena + (size_t)gates[g].out_slot[f] * slot_stride;
        for (int c = tid; c <= big; c += NT) {
            const int pp = c < big ? c / N : K, t = c < big ? c % N : 0;
            const int j = t == 0 ? 0 : N - t;
            const uint32_t* r0 = xbuf + 2 * pp * G::NP;
            uint32_t v0 = w_step<G>(r0, tf, nt, j, rns::P0, 0), v1 = w_step<G>(r0 + G::NP, tf, nt, j, rns::P1, 1);
            if (t != 0) {
                v0 = rns::negm(v0, rns::P0);
                v1 = rns::negm(v1, rns::P1);
            }
            out[c] = rns::to_torus(v0, v1);
        }
    }
}

// ------------------------------------------------------ BSK -> NTT domain
// block = (i, r); lanes (c, prime): residue of the mod-Q coefficient, to
// Montgomery form, forward NTT, canonical, times 1/N.
template <int N, int K, int E>
__global__ void __launch_bounds__(2 * (K + 1) * (N / E))
k_bsk_to_ntt(const uint64_t* __restrict__ coef, const uint32_t* __restrict__ tw, uint32_t ninv_r0, uint32_t ninv_r1,
             uint32_t* __restrict__ out) {
    using G = NttGeo<N, E>;
    static_assert(G::base_matches_geo(), "base<p> must be the index map the LDS-map proofs reason about");
    constexpr int NT = br_threads<N, K, E>();
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    uint32_t* xbuf = smem;
    uint32_t* zt_all = xbuf + 2 * (K + 1) * G::NP;
    const int tid = threadIdx.x, PQ = __builtin_amdgcn_readfirstlane(tid / G::T), tl = tid % G::T;
    const int P = PQ >> 1, q = PQ & 1;
    const uint32_t pm = rns::prime(q), pn = rns::pneg(q);
    const uint32_t r2 = q ? rns::R2_1 : rns::R2_0, ninv = q ? ninv_r1 : ninv_r0;
    for (int i = tid; i < 2 * N; i += NT) zt_all[i] = tw[i];
    __syncthreads();
    const size_t poly = (size_t)blockIdx.x * (K + 1) + P;  // blockIdx.x = i*(K+1) + r
    uint32_t x[E];
#pragma unroll
    for (int m = 0; m < E; ++m) x[m] = mont(rns::reduce64(coef[poly * N + G::template idx<0>(tl, m)], q), r2, pm, pn);
    forward_ntt<N, E>(x, xbuf + PQ * G::NP, zt_all + q * N, tl, pm, pn);
#pragma unroll
    for (int m = 0; m < E; ++m) out[(poly * 2 + q) * N + bsk_pos<N, E>(tl, m)] = mont(red1(red2(x[m], pm), pm), ninv, pm, pn);
}

// ------------------------------------------------ ring product (parity test)
// lanes (operand, prime); product of a, b in [0, Q) mod Q
template <int N, int E>
__global__ void __launch_bounds__(4 * (N / E))
k_ring_mul(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, const uint32_t* __restrict__ tw,
           uint32_t r2n0, uint32_t r2n1, uint64_t* __restrict__ out) {
    using G = NttGeo<N, E>;
    static_assert(G::base_matches_geo(), "base<p> must be the index map the LDS-map proofs reason about");
    constexpr int LAST = G::NPH - 1;
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    uint32_t* xbuf = smem;  // rows (operand, prime)
    uint32_t* zt_all = xbuf + 4 * G::NP;
    const int tid = threadIdx.x, PQ = __builtin_amdgcn_readfirstlane(tid / G::T), tl = tid % G::T;
    const int P = PQ >> 1, q = PQ & 1;
    const uint32_t pm = rns::prime(q), pn = rns::pneg(q);
    for (int i = tid; i < 2 * N; i += 4 * G::T) zt_all[i] = tw[i];
    __syncthreads();
    const uint32_t* zt = zt_all + q * N;
    const uint64_t* src = (P == 0 ? a : b) + (size_t)blockIdx.x * N;
    uint32_t x[E];
#pragma unroll
    for (int m = 0; m < E; ++m) x[m] = rns::reduce64(src[G::template idx<0>(tl, m)], q);
    uint32_t* row = xbuf + PQ * G::NP;
    forward_ntt<N, E>(x, row, zt, tl, pm, pn);
    __syncthreads();
#pragma unroll
    for (int m = 0; m < E; ++m) row[G::template at<G::XL>(G::template idx<LAST>(tl, m))] = x[m];
    __syncthreads();
    // a*b/R, then * R^2/N / R
    const uint32_t r2n = q ? r2n1 : r2n0;
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int pos = G::template at<G::XL>(G::template idx<LAST>(tl, m));
        const uint32_t u = red1(red2(xbuf[q * G::NP + pos], pm), pm);  // operand a, canonical
        x[m] = mont(mont_lazy(u, xbuf[(2 + q) * G::NP + pos], pm, pn), r2n, pm, pn);
    }
    inverse_ntt<N, E>(x, row, zt, tl, pm, pn);
    __syncthreads();
#pragma unroll
    for (int m = 0; m < E; ++m) row[G::template at<0>(G::template idx<0>(tl, m))] = red1(x[m], pm);
    __syncthreads();
    for (int c = tid; c < N; c += 4 * G::T)
        out[(size_t)blockIdx.x * N + c] = rns::crt(xbuf[G::template at<0>(c)], xbuf[G::NP + G::template at<0>(c)]);
}

// ================================================================== host side
template <int N, int K, int E>
static void set_smem_attr() {
    HIP_CHECK(hipFuncSetAttribute((const void*)k_blind_rotate<N, K, E>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)br_smem_bytes<N, K, E>()));
    HIP_CHECK(hipFuncSetAttribute((const void*)k_bsk_to_ntt<N, K, E>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)br_smem_bytes<N, K, E>()));
}

// run `body` with compile-time (N, K, E) matching the runtime parameters
template <class F>
static void dispatch(const Params& p, int E, F&& body) {
    auto pick = [&](auto n, auto k, auto e) {
        if (p.N == decltype(n)::value && p.k == decltype(k)::value && E == decltype(e)::value) {
            body(n, k, e);
            return true;
        }
        return false;
    };
    using I2048 = std::integral_constant<int, 2048>;
    using I1024 = std::integral_constant<int, 1024>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using E8 = std::integral_constant<int, 8>;
    using E16 = std::integral_constant<int, 16>;
    if (pick(I2048{}, I1{}, E16{}) || pick(I2048{}, I1{}, E8{})) return;
    if (pick(I1024{}, I2{}, E16{}) || pick(I1024{}, I2{}, E8{})) return;
    if (pick(I1024{}, I1{}, E16{}) || pick(I1024{}, I1{}, E8{})) return;
    throw Error(FR_ERR_INVALID, "device: no kernel variant for (N, k, E)");
}

void Device::init_rns() {
    // unrolled (k = 1) kernels keep three GGSW rows in registers: E = 8 only
    if (p_.bsk_unroll() == 2) e_ = e_small_ = 8;
    if (const char* ev = std::getenv("FR_LANE_ELEMS")) e_ = std::atoi(ev);
    if (const char* ev = std::getenv("FR_SMALL_LANE_ELEMS")) e_small_ = std::atoi(ev);
    if (const char* ev = std::getenv("FR_SMALL_BATCH")) small_batch_ = (size_t)std::atol(ev);
    if ((e_ != 8 && e_ != 16) || (e_small_ != 8 && e_small_ != 16))
        throw Error(FR_ERR_INVALID, "FR_LANE_ELEMS / FR_SMALL_LANE_ELEMS must be 8 or 16");
    for (int e : {8, 16})
        dispatch(p_, e, [&](auto n, auto k, auto ec) { set_smem_attr<decltype(n)::value, decltype(k)::value, decltype(ec)::value>(); });
    // Montgomery-form forward twiddles, per prime: zeta_q[k] * 2^32 mod p_q
    NttTables T(p_.N);
    std::vector<uint32_t> tw(2 * (size_t)p_.N);
    for (int q = 0; q < 2; ++q)
        for (int i = 0; i < p_.N; ++i) tw[(size_t)q * p_.N + i] = (uint32_t)(((uint64_t)T.zeta[q][i] << 32) % rns::prime(q));
    d_tw_.alloc(tw.size());
    HIP_CHECK(hipMemcpy(d_tw_.get(), tw.data(), 4 * tw.size(), hipMemcpyHostToDevice));
}

// BSK coefficients mod Q -> d_bsk_ (NTT domain)
void Device::upload_rns_bsk(const std::vector<uint64_t>& bsk) {
    gpu::DevBuf<uint64_t> coef(bsk.size());
    HIP_CHECK(hipMemcpy(coef.get(), bsk.data(), 8 * bsk.size(), hipMemcpyHostToDevice));
    d_bsk_.alloc(2 * bsk.size());  // two u32 residues per coefficient
    // 1/N in Montgomery form per prime
    uint32_t ninv_r[2];
    for (int q = 0; q < 2; ++q) ninv_r[q] = (uint32_t)((mod_inverse((uint64_t)p_.N, rns::prime(q)) << 32) % rns::prime(q));
    const int blocks = (int)p_.bsk_ggsw() * (p_.k + 1);
    dispatch(p_, e_, [&](auto n_, auto k_, auto e_c) {
        constexpr int N = decltype(n_)::value, K = decltype(k_)::value, E = decltype(e_c)::value;
        k_bsk_to_ntt<N, K, E><<<blocks, br_threads<N, K, E>(), br_smem_bytes<N, K, E>(), STREAM>>>(coef.get(), d_tw_.get(), ninv_r[0],
                                                                                                    ninv_r[1], d_bsk_.get());
    });
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(STREAM));
}

void Device::launch_br_rns(const DevGate* d_gates, const uint64_t* d_ks, size_t n, hipEvent_t ev_start, hipEvent_t ev_stop) {
    // small levels (at most one bootstrap per CU): more lanes per bootstrap for latency
    const int E = br_shape(n, false) == BrShape::Latency ? e_small_ : e_;
    dispatch(p_, E, [&](auto n_, auto k_, auto e_c) {
        constexpr int N = decltype(n_)::value, K = decltype(k_)::value, E = decltype(e_c)::value;
        hipExtLaunchKernelGGL(k_blind_rotate<N, K, E>, dim3((unsigned)n), dim3(br_threads<N, K, E>()),
                              (uint32_t)br_smem_bytes<N, K, E>(), STREAM, ev_start, ev_stop, 0, d_ks, p_.ks_stride(),
                              p_.n, d_gates, (const uint32_t*)d_bsk_.get(), (const uint32_t*)d_tw_.get(), d_arena_.get(),
                              p_.slot_stride());
    });
    HIP_CHECK(hipGetLastError());
}

void Device::ring_mul_host(const uint64_t* a, const uint64_t* b, size_t count, uint64_t* out) {
    if (p_.ring != FR_RING_RNS) throw Error(FR_ERR_INVALID, "ring_mul test hook: RNS ring only");
    const int N = p_.N;
    gpu::DevBuf<uint64_t> da(count * N), db(count * N), dout(count * N);
    HIP_CHECK(hipMemcpy(da.get(), a, 8 * count * N, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(db.get(), b, 8 * count * N, hipMemcpyHostToDevice));
    // R^2 / N mod p (Montgomery: turns mont(a, b) = ab/R into ab/N)
    uint32_t r2n[2];
    for (int q = 0; q < 2; ++q) {
        const uint64_t pq = rns::prime(q), r2 = q ? rns::R2_1 : rns::R2_0;
        r2n[q] = (uint32_t)(r2 * mod_inverse((uint64_t)N, pq) % pq);
    }
    dispatch(p_, e_, [&](auto n_, auto k_, auto e_c) {
        constexpr int NN = decltype(n_)::value, E = decltype(e_c)::value;
        (void)k_;
        const size_t sm = 4 * (4 * (size_t)NttGeo<NN, E>::NP + 2 * (size_t)NN);
        HIP_CHECK(hipFuncSetAttribute((const void*)k_ring_mul<NN, E>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm));
        k_ring_mul<NN, E><<<(unsigned)count, 4 * (NN / E), sm, STREAM>>>(da.get(), db.get(), d_tw_.get(), r2n[0], r2n[1], dout.get());
    });
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(STREAM));
    HIP_CHECK(hipMemcpy(out, dout.get(), 8 * count * N, hipMemcpyDeviceToHost));
}

}  // namespace fr
