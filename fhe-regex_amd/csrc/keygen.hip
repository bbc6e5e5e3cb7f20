// Server-key generation on the device (the reference's
// ServerKey::new at src/regex/engine.rs:252 and gen_keys_radix at
// src/regex/ciphertext.rs:44).  Bit-identical to keys.cpp's gen_ksk +
// gen_bsk_torus followed by fft::bsk_to_fourier (and therefore to the oracle's
// keygen): the same ChaCha20 words (chacha.h) for every mask, exact mod-2^64
// sums for the bodies, the same host Box-Muller noise (uploaded), and the same
// butterfly sequence for the Fourier transform.
//
// Kernels (all integer / f64 add-and-multiply work, HBM-bound or LDS-bound):
//   k_gen_ksk      one wave per KSK row (kN * ks_level rows): masks from ChaCha
//                  blocks, <mask, s_small> reduced over the wave, + s_big[i] *
//                  2^(64 - B(j+1)) + noise
//   k_gen_bsk      one workgroup per GGSW row (w, r): masks A_j from ChaCha into
//                  LDS, body = sum_j A_j * S_j (negacyclic, binary S: one
//                  add/sub per set bit of S per coefficient) + noise, gadget m_w
//                  2^(64 - pbs_base_log) on coefficient 0 of component r; COMPACT
//                  (keys.h): rows r < k carry the gadget in the body, -m_w g S_r
//   k_expand_ksk   compact key load, one wave per KSK row: the mask words from ChaCha
//                  blocks of the public mask key, the body from the uploaded blob
//   k_expand_rows  the same for one GLWE row per workgroup: k mask polynomials and the body
//                  -- a GGSW row (w, r) of the BSK with the blob's u64 body, or a row of a
//                  compact packing key with its 40-bit body from the two planes.  Both are
//                  pure store streams, 16 bytes a store
//   k_gather_planes40  the planes of a compact packing key back from its resident rows
//   k_expand_blocks  compact content, one workgroup per LWE block: the mask words from
//                  ChaCha blocks of the blob's mask key straight into the block's arena
//                  slot, the body from the staged bodies; the same 16-byte store stream
//   k_bsk_fourier  one workgroup per polynomial: fold, forward negacyclic FFT in
//                  LDS (fft.h butterflies, host twiddles), scale 2^-log2(M),
//                  written in the lane layouts of the blind-rotation kernels
//                  (E = 4; k = 2 also E = 8)
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "chacha.h"
#include "device_impl.h"
#include "fft.h"
#include "geo.h"
#include "keys.h"

namespace fr {

// u64 number 8*blk + q of a ChaCha stream: words (2q, 2q+1) of block blk
__device__ __forceinline__ uint64_t chacha_u64(const uint32_t* w, int q) {
    return (uint64_t)w[2 * q] | ((uint64_t)w[2 * q + 1] << 32);
}

// The generator key (RngKey, chacha.h) reaches every kernel below by value: a
// kernel argument is wave-uniform, so its 8 words are scalar operands of the
// ChaCha rounds and are never written to global memory.

// ksk[row][t], row = i * L + j; masks are u64 numbers row * n + t of STREAM_KSK_MASK
__global__ void __launch_bounds__(64) k_gen_ksk(RngKey key, int n, int L, int B, const uint64_t* __restrict__ s_small,
                                                const uint64_t* __restrict__ s_big, const int64_t* __restrict__ noise,
                                                uint64_t* __restrict__ ksk) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const int i = row / L, j = row % L;
    const uint64_t first = (uint64_t)row * n, last = first + n;
    uint64_t* o = ksk + (size_t)row * (n + 1);
    uint64_t acc = 0;
    for (uint64_t b = (first >> 3) + lane; b <= ((last - 1) >> 3); b += 64) {
        uint32_t w[16];
        chacha_block(key, STREAM_KSK_MASK, b, w);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const uint64_t idx = b * 8 + q;
            if (idx >= first && idx < last) {
                const int t = (int)(idx - first);
                const uint64_t v = chacha_u64(w, q);
                o[t] = v;
                acc += v * s_small[t];
            }
        }
    }
    // wave sum mod 2^64 (order-free)
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) o[n] = acc + (s_big[i] << (64 - B * (j + 1))) + (uint64_t)noise[row];
}

// The masks of one GLWE row and their exact key product, shared by k_gen_bsk and k_gen_pksk:
// mask polynomial j < k is u64 numbers base + j N + t of `stream` (N % 8 == 0: whole ChaCha
// blocks), stored to row[j N + t] (plus `gadget` on coefficient 0 of polynomial gj, if gj >= 0,
// after the product used the mask); acc[q] += (sum_j A_j S_j)[tid + 256 q], negacyclic, binary
// S: one add / sub per set bit of S per coefficient.  256 threads; LDS: A (N u64), sbits.
template <int N>
__device__ __forceinline__ void glwe_masks_product(const RngKey& key, uint64_t stream, uint64_t base, int k,
                                                   const uint64_t* __restrict__ s_big, int gj, uint64_t gadget,
                                                   uint64_t* __restrict__ row, uint64_t* A, uint32_t* sbits,
                                                   uint64_t (&acc)[N / 256]) {
    constexpr int PER = N / 256;
    const int tid = threadIdx.x;
    for (int j = 0; j < k; ++j) {
        const uint64_t bj = base + (uint64_t)j * N;
        for (int b = tid; b < N / 8; b += 256) {
            uint32_t wd[16];
            chacha_block(key, stream, (bj >> 3) + b, wd);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                uint64_t v = chacha_u64(wd, q);
                A[8 * b + q] = v;
                if (j == gj && b == 0 && q == 0) v += gadget;
                row[(size_t)j * N + 8 * b + q] = v;
            }
        }
        const uint64_t* S = s_big + (size_t)j * N;
        for (int x = tid; x < N / 32; x += 256) {
            uint32_t m = 0;
            for (int y = 0; y < 32; ++y) m |= (uint32_t)(S[32 * x + y] & 1) << y;
            sbits[x] = m;
        }
        __syncthreads();
        // body += X^u A for every set bit u of S_j: coefficient t gets A[t - u]
        // (t >= u) or -A[t - u + N] (wrapped)
        for (int x = 0; x < N / 32; ++x) {
            uint32_t m = sbits[x];
            while (m) {
                const int u = 32 * x + __builtin_ctz(m);
                m &= m - 1;
#pragma unroll
                for (int q = 0; q < PER; ++q) {
                    const int t = tid + 256 * q;
                    const int d = t - u;
                    const uint64_t a = A[d >= 0 ? d : d + N];
                    acc[q] = d >= 0 ? acc[q] + a : acc[q] - a;
                }
            }
        }
        __syncthreads();
    }
}

// one GGSW row (w, r) of the torus BSK [w][r][c][coef]; 256 threads, N / 256
// coefficients per thread; LDS: the mask polynomial A_j (N u64).  COMPACT: `key` is the
// public mask key, so no mask word may carry the gadget (word - ChaCha word would show
// m_w): rows r < k subtract it from the body at every set bit of S_r instead.
template <int N, bool COMPACT>
__global__ void __launch_bounds__(256) k_gen_bsk(RngKey key, int k,const uint64_t* __restrict__ s_big,
                                                 const uint8_t* __restrict__ msg, const int32_t* __restrict__ noise,
                                                 uint64_t gadget, uint64_t* __restrict__ bsk) {
    constexpr int PER = N / 256;
    __shared__ uint64_t A[N];
    __shared__ uint32_t sbits[N / 32];
    const int kp1 = k + 1, tid = threadIdx.x;
    const int w = blockIdx.x / kp1, r = blockIdx.x % kp1;
    uint64_t* row = bsk + ((size_t)w * kp1 + r) * kp1 * N;
    uint64_t acc[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) acc[q] = 0;
    // the gadget lands on coefficient 0 of component r (r < k: a mask polynomial)
    glwe_masks_product<N>(key, STREAM_BSK_MASK, ((uint64_t)w * kp1 + r) * k * N, k, s_big,
                          !COMPACT && msg[w] ? r : -1, gadget, row, A, sbits, acc);
    const int32_t* e = noise + ((size_t)w * kp1 + r) * N;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int t = tid + 256 * q;
        uint64_t v = acc[q] + (uint64_t)(int64_t)e[t];
        if (r == k && t == 0 && msg[w]) v += gadget;
        if (COMPACT && r < k && msg[w]) v -= gadget * (s_big[(size_t)r * N + t] & 1);
        row[(size_t)k * N + t] = v;
    }
}

// one row 3 i + l of the packing key (keys.h): k mask polynomials from STREAM_PKSK_MASK, body =
// sum_j A_j S_j + noise, + s_big[i] 2^(64 - PK_BASE_LOG (l + 1)) on coefficient 0.  grid = rows of
// (k + 1) N words, so every store is inside the key.  COMPACT (keys.h): `key` is the public mask
// key (the message sits in the body, so no mask word carries a secret) and the epilogue rounds
// the body to its top 40 bits, pk_round40(v) << 24
template <int N, bool COMPACT>
__global__ void __launch_bounds__(256) k_gen_pksk(RngKey key, int k, const uint64_t* __restrict__ s_big,
                                                  const int32_t* __restrict__ noise, uint64_t* __restrict__ pksk) {
    constexpr int PER = N / 256;
    __shared__ uint64_t A[N];
    __shared__ uint32_t sbits[N / 32];
    const int tid = threadIdx.x;
    const size_t r = blockIdx.x;
    const int i = (int)(r / PK_LEVELS), l = (int)(r % PK_LEVELS);
    uint64_t* row = pksk + r * (size_t)(k + 1) * N;
    uint64_t acc[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) acc[q] = 0;
    glwe_masks_product<N>(key, STREAM_PKSK_MASK, (uint64_t)r * k * N, k, s_big, -1, 0, row, A, sbits, acc);
    const int32_t* e = noise + r * N;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int t = tid + 256 * q;
        uint64_t v = acc[q] + (uint64_t)(int64_t)e[t];
        if (t == 0) v += (s_big[i] & 1) << (64 - PK_BASE_LOG * (l + 1));
        if (COMPACT) v = ((v + ((uint64_t)1 << (PKC_DROP_BITS - 1))) >> PKC_DROP_BITS) << PKC_DROP_BITS;  // pk_round40
        row[(size_t)k * N + t] = v;
    }
}

// Compact-key expansion: masks are u64 numbers of the public mask key's streams at the
// generator's indices, bodies come from the blob.  No sums, no LDS: store streams.

// The u64 of ChaCha block b in a KSK row whose first mask word is stream number `first`:
// word q is the row's element t0 + q, t0 = 8b - first (negative or past n where the block
// straddles a neighbouring row: first = row * n is no multiple of 8).  The element's
// address is ksk + row + 8b + q words, so pairs starting at a q of the row's parity are
// 16-byte aligned and go out as one store; ODD rows store q = 0 and q = 7 alone.
template <int ODD>
__device__ __forceinline__ void expand_ksk_block(uint64_t* __restrict__ o, const uint32_t* w, int t0, int n) {
    auto one = [&](int q) {
        const int t = t0 + q;
        if (t >= 0 && t < n) o[t] = chacha_u64(w, q);
    };
    if (ODD) one(0);
#pragma unroll
    for (int q = ODD; q + 1 < 8; q += 2) {
        const int t = t0 + q;
        if (t >= 0 && t + 1 < n) {
            *reinterpret_cast<ulonglong2*>(o + t) = make_ulonglong2(chacha_u64(w, q), chacha_u64(w, q + 1));
        } else {
            one(q);
            one(q + 1);
        }
    }
    if (ODD) one(7);
}

// ksk[row][t] for t < n from the mask key, ksk[row][n] = body[row]; grid = rows, so every
// store is inside row's n + 1 words
__global__ void __launch_bounds__(64) k_expand_ksk(RngKey mask_key, int n, const uint64_t* __restrict__ body,
                                                   uint64_t* __restrict__ ksk) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const uint64_t first = (uint64_t)row * n, last = first + n;
    uint64_t* o = ksk + (size_t)row * (n + 1);
    for (uint64_t b = (first >> 3) + lane; b <= ((last - 1) >> 3); b += 64) {
        uint32_t w[16];
        chacha_block(mask_key, STREAM_KSK_MASK, b, w);
        const int t0 = (int)((int64_t)(b * 8) - (int64_t)first);
        if (row & 1) expand_ksk_block<1>(o, w, t0, n);
        else expand_ksk_block<0>(o, w, t0, n);
    }
    if (lane == 0) o[n] = body[row];
}

// Where the body polynomial of an expanded row comes from: row(gr, dst) writes the N words of
// row gr's body to dst (16-byte aligned) with 16-byte stores, 256 threads.
// the compact server key's blob: the u64 bodies as they are
template <int N>
struct BodyWords {
    const uint64_t* body;  // [rows][N], 16-byte aligned
    __device__ __forceinline__ void row(size_t gr, uint64_t* __restrict__ dst) const {
        const ulonglong2* src = reinterpret_cast<const ulonglong2*>(body + gr * N);
        ulonglong2* d = reinterpret_cast<ulonglong2*>(dst);
        for (int x = threadIdx.x; x < N / 2; x += 256) d[x] = src[x];
    }
};
// the compact packing key's planes (keys.h): word t = b40 << 24, b40 = hi[t] << 8 | lo[t]; four
// coefficients per thread step, 16 bytes of the high plane and 4 of the low into two stores
template <int N>
struct BodyPlanes40 {
    const uint32_t* hi;  // [rows][N], 16-byte aligned
    const uint8_t* lo;   // [rows][N], 4-byte aligned
    __device__ __forceinline__ void row(size_t gr, uint64_t* __restrict__ dst) const {
        const uint4* h4 = reinterpret_cast<const uint4*>(hi + gr * N);
        const uint32_t* l4 = reinterpret_cast<const uint32_t*>(lo + gr * N);
        ulonglong2* d = reinterpret_cast<ulonglong2*>(dst);
        for (int x = threadIdx.x; x < N / 4; x += 256) {
            const uint4 h = h4[x];
            const uint32_t l = l4[x];
            auto word = [](uint32_t hw, uint32_t lb) { return ((uint64_t)hw << 32) | ((uint64_t)lb << PKC_DROP_BITS); };
            d[2 * x] = make_ulonglong2(word(h.x, l & 0xFF), word(h.y, (l >> 8) & 0xFF));
            d[2 * x + 1] = make_ulonglong2(word(h.z, (l >> 16) & 0xFF), word(h.w, l >> 24));
        }
    }
};

// one GLWE row of a key of rows [k mask polynomials][body] -- a GGSW row (w, r) of the torus
// BSK (STREAM_BSK_MASK, BodyWords) or a row of the packing key (STREAM_PKSK_MASK,
// BodyPlanes40): the masks are the kN / 8 whole ChaCha blocks from u64 number gr k N of
// MASK_STREAM under the mask key, 64 aligned bytes each, the body comes from `body`; grid = rows of
// (k + 1) N words, so every store is inside the key
template <int N, uint64_t MASK_STREAM, class Body>
__global__ void __launch_bounds__(256) k_expand_rows(RngKey mask_key, int k, Body body, uint64_t* __restrict__ key) {
    const int tid = threadIdx.x;
    const size_t gr = blockIdx.x;  // BSK: w * (k + 1) + r
    uint64_t* row = key + gr * (size_t)(k + 1) * N;
    const uint64_t base = gr * (uint64_t)k * N;  // mask polynomial j starts at base + j N
    for (int b = tid; b < k * (N / 8); b += 256) {
        uint32_t wd[16];
        chacha_block(mask_key, MASK_STREAM, (base >> 3) + b, wd);
        ulonglong2* o = reinterpret_cast<ulonglong2*>(row + 8 * (size_t)b);
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = make_ulonglong2(chacha_u64(wd, 2 * q), chacha_u64(wd, 2 * q + 1));
    }
    body.row(gr, row + (size_t)k * N);
}

// the two planes of a compact packing key from its resident rows (export): one workgroup per
// row, four body words per thread step into 16 bytes of the high plane and 4 of the low; grid
// = rows, so every store is inside the planes' 5 rows N bytes
template <int N>
__global__ void __launch_bounds__(256) k_gather_planes40(int k, const uint64_t* __restrict__ key,
                                                         uint32_t* __restrict__ hi, uint8_t* __restrict__ lo) {
    const size_t gr = blockIdx.x;
    const ulonglong2* src = reinterpret_cast<const ulonglong2*>(key + (gr * (size_t)(k + 1) + k) * N);
    uint4* h4 = reinterpret_cast<uint4*>(hi + gr * N);
    uint32_t* l4 = reinterpret_cast<uint32_t*>(lo + gr * N);
    for (int x = threadIdx.x; x < N / 4; x += 256) {
        const ulonglong2 a = src[2 * x], b = src[2 * x + 1];
        auto low = [](uint64_t v) { return (uint32_t)(v >> PKC_DROP_BITS) & 0xFF; };
        h4[x] = make_uint4((uint32_t)(a.x >> 32), (uint32_t)(a.y >> 32), (uint32_t)(b.x >> 32), (uint32_t)(b.y >> 32));
        l4[x] = low(a.x) | (low(a.y) << 8) | (low(b.x) << 16) | (low(b.y) << 24);
    }
}

// fold + forward FFT + fourier_key_scale of one polynomial, written in the lane layouts of
// the E = 4 and E = 8 kernels ([poly][m][lane], slot of (lane, m): fft_key_slot of geo.h; a
// null output is skipped)
template <int N>
__global__ void __launch_bounds__(256) k_bsk_fourier(const uint64_t* __restrict__ bsk, const double2* __restrict__ tw,
                                                     double2* __restrict__ out4, double2* __restrict__ out8) {
    constexpr int M = N / 2;
    constexpr int LOG = __builtin_ctz(M);
    __shared__ double2 z[M];
    const int tid = threadIdx.x;
    const size_t p = blockIdx.x;
    const uint64_t* a = bsk + p * N;
    for (int i = tid; i < M; i += 256) z[i] = make_double2((double)(int64_t)a[i], (double)(int64_t)a[i + M]);
    __syncthreads();
    for (int s = 0; s < LOG; ++s) {
        const int h = M >> (s + 1);
        for (int bi = tid; bi < M / 2; bi += 256) {
            const int b = bi / h, j = b * 2 * h + bi % h;
            const double2 c = tw[(1 << s) + b];
            double2 lo = z[j], hi = z[j + h];
            fft::fwd_bf(lo.x, lo.y, hi.x, hi.y, c.x, c.y);
            z[j] = lo;
            z[j + h] = hi;
        }
        __syncthreads();
    }
    const double scale = fft::fourier_key_scale(LOG);  // 1/M and the accumulator unit (fft.h), exact
    for (int idx = tid; idx < M; idx += 256) {
        if (out4) {
            const double2 v = z[fft_key_slot(LOG, 2, idx % (M / 4), idx / (M / 4))];
            out4[p * M + idx] = make_double2(v.x * scale, v.y * scale);
        }
        if (out8) {
            const double2 v = z[fft_key_slot(LOG, 3, idx % (M / 8), idx / (M / 8))];
            out8[p * M + idx] = make_double2(v.x * scale, v.y * scale);
        }
    }
}

// fresh LWE encryptions of block messages under the big key straight into
// arena slots (encrypt_str, src/regex/ciphertext.rs:32-40):
// one wave per block; masks are u64 numbers qb * kN + t of STREAM_ENC_MASK
// (kN % 8 == 0: whole ChaCha blocks), body = <mask, s_big> + m 2^59 + noise
__global__ void __launch_bounds__(64) k_encrypt_blocks(RngKey key, int big,const uint64_t* __restrict__ s_big,
                                                       const uint8_t* __restrict__ msgs,
                                                       const int64_t* __restrict__ noise, uint64_t first_block,
                                                       const int* __restrict__ slots, int stride,
                                                       uint64_t* __restrict__ arena) {
    const int q = blockIdx.x, lane = threadIdx.x;
    const uint64_t qb = first_block + q;
    uint64_t* o = arena + (size_t)slots[q] * stride;
    uint64_t acc = 0;
    for (int b = lane; b < big / 8; b += 64) {
        uint32_t w[16];
        chacha_block(key, STREAM_ENC_MASK, qb * (uint64_t)(big / 8) + b, w);
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const uint64_t v = chacha_u64(w, x);
            o[8 * b + x] = v;
            acc += v * s_big[8 * b + x];
        }
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) o[big] = acc + ((uint64_t)msgs[q] << DELTA_LOG) + (uint64_t)noise[q];
}

void Device::encrypt_to_slots(const ClientKey& ck, const uint8_t* msgs, size_t count, const RngKey& key,
                              uint64_t first_block, const int* slots) {
    if (!count) return;
    const int big = p_.big();
    if (big % 8) throw Error(FR_ERR_INVALID, "device encryption: kN must be a multiple of 8");
    if (ck.s_big.size() != (size_t)big) throw Error(FR_ERR_INVALID, "device encryption: key size");
    for (size_t i = 0; i < count; ++i)
        if (slots[i] < 0 || (size_t)slots[i] >= next_slot_) throw Error(FR_ERR_INVALID, "device encryption: slot");
    std::vector<int64_t> noise;
    enc_noise(p_, key, first_block, count, noise);
    const hipStream_t s = cur().stream.get();
    gpu::DevBuf<uint64_t> d_sb((size_t)big);
    gpu::DevBuf<uint8_t> d_m(count);
    gpu::DevBuf<int64_t> d_n(count);
    gpu::DevBuf<int> d_sl(count);
    HIP_CHECK(hipMemcpyAsync(d_sb.get(), ck.s_big.data(), 8 * (size_t)big, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_m.get(), msgs, count, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_n.get(), noise.data(), 8 * count, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_sl.get(), slots, 4 * count, hipMemcpyHostToDevice, s));
    k_encrypt_blocks<<<(unsigned)count, 64, 0, s>>>(key, big, d_sb.get(), d_m.get(), d_n.get(), first_block, d_sl.get(),
                                                   p_.slot_stride(), d_arena_.get());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));  // the temporaries go once the kernel has run
}

// Compact content (keys.h): the LWEs of `grid` blocks rebuilt in their arena slots, one
// workgroup per LWE.  Mask word t of block q is u64 number (first_block + q) kN + t of
// STREAM_ENC_MASK under the public mask key (k_encrypt_blocks's indices; kN % 8 == 0: whole
// ChaCha blocks); thread t owns ChaCha block (first_block + q) kN / 8 + t, 64 aligned bytes
// of the slot (slot stride: a multiple of 64 B), stored 16 bytes at a time as k_expand_rows
// does.  The body word comes from the staged bodies.  Every store is inside the slot's
// big + 1 words; the host checked slots[q] < next_slot_.
__global__ void __launch_bounds__(256) k_expand_blocks(RngKey mask_key, int big, uint64_t first_block,
                                                       const uint64_t* __restrict__ bodies,
                                                       const int* __restrict__ slots, int stride,
                                                       uint64_t* __restrict__ arena) {
    const int q = blockIdx.x, tid = threadIdx.x;
    const uint64_t base = (first_block + q) * (uint64_t)(big / 8);
    uint64_t* o = arena + (size_t)slots[q] * stride;
    for (int b = tid; b < big / 8; b += 256) {
        uint32_t w[16];
        chacha_block(mask_key, STREAM_ENC_MASK, base + b, w);
        ulonglong2* d = reinterpret_cast<ulonglong2*>(o + 8 * (size_t)b);
#pragma unroll
        for (int x = 0; x < 4; ++x) d[x] = make_ulonglong2(chacha_u64(w, 2 * x), chacha_u64(w, 2 * x + 1));
    }
    if (tid == 0) o[big] = bodies[q];
}

Slots Device::expand_to_slots(const RngKey& mask_key, uint64_t first_block, const uint8_t* bodies, size_t count) {
    Slots slots(*this);
    if (!count) return slots;
    const int big = p_.big();
    if (big % 8) throw Error(FR_ERR_INVALID, "device expansion: kN must be a multiple of 8");
    if (lane_ != 0) throw Error(FR_ERR_INVALID, "device expansion: lane 0 only");
    if (count > (size_t)1 << 30) throw Error(FR_ERR_INVALID, "device expansion: too many blocks");
    // every slot first: alloc_slot may grow the arena, which moves it (ensure_arena)
    slots.alloc(count);
    // staging: the bodies [count] u64, then the slot list [count] int, in one H2D copy
    const size_t need = 12 * count;
    const hipStream_t s = STREAM;
    xstage_.reserve(need, 12 * 4096, s);
    uint8_t* h = xstage_.acquire();
    std::memcpy(h, bodies, 8 * count);
    std::memcpy(h + 8 * count, slots.data(), 4 * count);
    xstage_.commit(need, s);
    // the device side is reused in stream order: the next call's copy runs after this kernel
    gpu::Event t0, t1;
    if (profiling_) {
        t0 = take_event();
        t1 = take_event();
        HIP_CHECK(hipEventRecord(t0.get(), s));
    }
    const uint8_t* d = xstage_.device();
    k_expand_blocks<<<(unsigned)count, 256, 0, s>>>(mask_key, big, first_block, (const uint64_t*)d,
                                                   (const int*)(d + 8 * count), p_.slot_stride(), d_arena_.get());
    HIP_CHECK(hipGetLastError());
    if (profiling_) {
        // the probe's figure (fr_device_timers_content): a profiled call waits for its kernel
        HIP_CHECK(hipEventRecord(t1.get(), s));
        HIP_CHECK(hipEventSynchronize(t1.get()));
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, t0.get(), t1.get()));
        expand_ms_ = ms;
        event_pool_.push_back(std::move(t0));
        event_pool_.push_back(std::move(t1));
    }
    return slots;
}

static void need_device_keygen_point(const Params& p, const char* what) {
    if (p.ring != FR_RING_FFT || !((p.N == 2048 && p.k == 1) || (p.N == 1024 && p.k == 2)))
        throw Error(FR_ERR_INVALID, std::string(what) + ": FFT ring, (k, N) in {(1, 2048), (2, 1024)}");
}

// Fourier BSK in the lane layouts of the shapes in use (E = 4, and the throughput shape's)
void Device::build_fourier_bsk() {
    const int N = p_.N, M = N / 2, kp1 = p_.k + 1;
    const size_t bsk_polys = p_.bsk_ggsw() * kp1 * kp1;
    const hipStream_t s = cur().stream.get();
    for (int E : {4, 8}) {
        gpu::DevBuf<double>& dst = d_fbsk_[fbsk_index(E)];
        dst.reset();
        if (fbsk_needed(E)) dst.alloc(2 * bsk_polys * M);
    }
    double2 *o4 = (double2*)d_fbsk_[0].get(), *o8 = (double2*)d_fbsk_[1].get();
    if (N == 2048)
        k_bsk_fourier<2048><<<(unsigned)bsk_polys, 256, 0, s>>>(d_tbsk_.get(), (const double2*)d_ftw_.get(), o4, o8);
    else
        k_bsk_fourier<1024><<<(unsigned)bsk_polys, 256, 0, s>>>(d_tbsk_.get(), (const double2*)d_ftw_.get(), o4, o8);
    HIP_CHECK(hipGetLastError());
}

void Device::gen_server_key(const ClientKey& ck, const RngKey& key, const RngKey* mask_key) {
    need_device_keygen_point(p_, "device keygen");
    const int N = p_.N, kp1 = p_.k + 1, n = p_.n, L = p_.ks_level;
    const size_t rows = (size_t)p_.big() * L, nw = p_.bsk_ggsw();
    const bool compact = mask_key != nullptr;
    const RngKey& kkey = compact ? *mask_key : key;  // the key the kernels see
    Replacing key_guard([this] { drop_server_key(); });
    // host: the noise draws and per-GGSW messages
    std::vector<int64_t> ksk_noise;
    std::vector<int32_t> bsk_noise;
    gen_ksk_noise(p_, key, ksk_noise);
    gen_bsk_noise_torus(p_, key, bsk_noise);
    const std::vector<uint8_t> msg = ggsw_messages(p_, ck);

    const hipStream_t s = cur().stream.get();
    gpu::DevBuf<uint64_t> d_ss(ck.s_small.size()), d_sb(ck.s_big.size());
    gpu::DevBuf<int64_t> d_kn(ksk_noise.size());
    gpu::DevBuf<int32_t> d_bn(bsk_noise.size());
    gpu::DevBuf<uint8_t> d_msg(msg.size());
    HIP_CHECK(hipMemcpyAsync(d_ss.get(), ck.s_small.data(), 8 * ck.s_small.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_sb.get(), ck.s_big.data(), 8 * ck.s_big.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_kn.get(), ksk_noise.data(), 8 * ksk_noise.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_bn.get(), bsk_noise.data(), 4 * bsk_noise.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_msg.get(), msg.data(), msg.size(), hipMemcpyHostToDevice, s));

    // KSK (torus) and its byte limbs
    ksk_.alloc_rows((int)rows, n + 1);
    k_gen_ksk<<<(unsigned)rows, 64, 0, s>>>(kkey, n, L, p_.ks_base_log, d_ss.get(), d_sb.get(), d_kn.get(), ksk_.rows.get());
    HIP_CHECK(hipGetLastError());
    build_limbs(ksk_);

    // torus BSK, kept for export
    d_tbsk_.alloc(p_.bsk_len());
    const uint64_t gadget = 1ULL << (64 - p_.pbs_base_log);
    const unsigned grid = (unsigned)(nw * kp1);
    const uint64_t* sb = d_sb.get();
    const uint8_t* m = d_msg.get();
    const int32_t* bn = d_bn.get();
    uint64_t* tbsk = d_tbsk_.get();
    if (N == 2048 && !compact) k_gen_bsk<2048, false><<<grid, 256, 0, s>>>(kkey, p_.k, sb, m, bn, gadget, tbsk);
    else if (N == 2048) k_gen_bsk<2048, true><<<grid, 256, 0, s>>>(kkey, p_.k, sb, m, bn, gadget, tbsk);
    else if (!compact) k_gen_bsk<1024, false><<<grid, 256, 0, s>>>(kkey, p_.k, sb, m, bn, gadget, tbsk);
    else k_gen_bsk<1024, true><<<grid, 256, 0, s>>>(kkey, p_.k, sb, m, bn, gadget, tbsk);
    HIP_CHECK(hipGetLastError());

    build_fourier_bsk();
    HIP_CHECK(hipStreamSynchronize(s));
    key_guard.dismiss();
}

void Device::load_server_key_compact(const RngKey& mask_key, const uint8_t* bodies) {
    need_device_keygen_point(p_, "device load of a compact server key");
    const int N = p_.N, kp1 = p_.k + 1, n = p_.n;
    const size_t rows = compact_ksk_bodies(p_), brows = p_.bsk_ggsw() * kp1, words = rows + compact_bsk_bodies(p_);
    // the BSK bodies follow the KSK bodies in one staging buffer and are read 16 bytes a lane
    if (rows % 2 || N % 8) throw Error(FR_ERR_INVALID, "device load of a compact server key: alignment");
    Replacing key_guard([this] { drop_server_key(); });
    const hipStream_t s = cur().stream.get();
    gpu::DevBuf<uint64_t> d_body(words);
    StageTimer<5> timer(profiling_ != 0, s);
    ksk_.alloc_rows((int)rows, n + 1);
    d_tbsk_.alloc(p_.bsk_len());
    timer.mark(0);
    HIP_CHECK(hipMemcpyAsync(d_body.get(), bodies, 8 * words, hipMemcpyHostToDevice, s));
    timer.mark(1);
    k_expand_ksk<<<(unsigned)rows, 64, 0, s>>>(mask_key, n, d_body.get(), ksk_.rows.get());
    HIP_CHECK(hipGetLastError());
    timer.mark(2);
    if (N == 2048)
        k_expand_rows<2048, STREAM_BSK_MASK><<<(unsigned)brows, 256, 0, s>>>(
            mask_key, p_.k, BodyWords<2048>{d_body.get() + rows}, d_tbsk_.get());
    else
        k_expand_rows<1024, STREAM_BSK_MASK><<<(unsigned)brows, 256, 0, s>>>(
            mask_key, p_.k, BodyWords<1024>{d_body.get() + rows}, d_tbsk_.get());
    HIP_CHECK(hipGetLastError());
    timer.mark(3);
    build_limbs(ksk_);
    timer.mark(4);
    build_fourier_bsk();
    timer.mark(5);
    HIP_CHECK(hipStreamSynchronize(s));
    timer.read(key_load_ms_);
    key_guard.dismiss();
}

// Packing key on the device: the torus rows stay for download_packing_key (as the torus BSK
// does), the byte limbs are the MFMA operand of pack_bools
void Device::gen_packing_key(const ClientKey& ck, const RngKey& mask_key, const RngKey& noise_key, bool compact) {
    if (!((p_.N == 2048 && p_.k == 1) || (p_.N == 1024 && p_.k == 2)))
        throw Error(FR_ERR_INVALID, "device packing keygen: (k, N) in {(1, 2048), (2, 1024)}");
    if (ck.s_big.size() != (size_t)p_.big()) throw Error(FR_ERR_INVALID, "device packing keygen: key size");
    const size_t rows = pk_rows(p_);
    Replacing key_guard([this] { drop_packing_key(); });
    // host: the noise under the secret key; the kernel sees the mask key alone
    std::vector<int32_t> noise;
    gen_pksk_noise(p_, noise_key, noise);
    const hipStream_t s = cur().stream.get();
    gpu::DevBuf<uint64_t> d_sb(ck.s_big.size());
    gpu::DevBuf<int32_t> d_n(noise.size());
    HIP_CHECK(hipMemcpyAsync(d_sb.get(), ck.s_big.data(), 8 * ck.s_big.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_n.get(), noise.data(), 4 * noise.size(), hipMemcpyHostToDevice, s));
    pksk_.alloc_rows((int)rows, (int)pk_row_words(p_));
    const unsigned grid = (unsigned)rows;
    const uint64_t* sb = d_sb.get();
    const int32_t* e = d_n.get();
    uint64_t* out = pksk_.rows.get();
    if (p_.N == 2048 && !compact) k_gen_pksk<2048, false><<<grid, 256, 0, s>>>(mask_key, p_.k, sb, e, out);
    else if (p_.N == 2048) k_gen_pksk<2048, true><<<grid, 256, 0, s>>>(mask_key, p_.k, sb, e, out);
    else if (!compact) k_gen_pksk<1024, false><<<grid, 256, 0, s>>>(mask_key, p_.k, sb, e, out);
    else k_gen_pksk<1024, true><<<grid, 256, 0, s>>>(mask_key, p_.k, sb, e, out);
    HIP_CHECK(hipGetLastError());
    build_limbs(pksk_);
    HIP_CHECK(hipStreamSynchronize(s));  // the temporaries go once the kernels have run
    key_guard.dismiss();
}

static void need_pk_compact_point(const Params& p, const char* what) {
    if (p.N != 2048 && p.N != 1024) throw Error(FR_ERR_INVALID, std::string(what) + ": N in {1024, 2048}");
}

void Device::load_packing_key_compact(const RngKey& mask_key, const uint8_t* planes) {
    need_pk_compact_point(p_, "device load of a compact packing key");
    const size_t rows = pk_rows(p_), N = (size_t)p_.N, bytes = pk_compact_planes(p_);
    Replacing key_guard([this] { drop_packing_key(); });
    const hipStream_t s = cur().stream.get();
    // hipMalloc's alignment; the low plane follows 4 rows N bytes of the high one: 16-byte aligned
    gpu::DevBuf<uint8_t> d_planes(bytes);
    StageTimer<3> timer(profiling_ != 0, s);
    pksk_.alloc_rows((int)rows, (int)pk_row_words(p_));
    timer.mark(0);
    HIP_CHECK(hipMemcpyAsync(d_planes.get(), planes, bytes, hipMemcpyHostToDevice, s));
    timer.mark(1);
    const uint32_t* hi = reinterpret_cast<const uint32_t*>(d_planes.get());
    const uint8_t* lo = d_planes.get() + 4 * rows * N;
    if (N == 2048)
        k_expand_rows<2048, STREAM_PKSK_MASK><<<(unsigned)rows, 256, 0, s>>>(mask_key, p_.k, BodyPlanes40<2048>{hi, lo},
                                                                            pksk_.rows.get());
    else
        k_expand_rows<1024, STREAM_PKSK_MASK><<<(unsigned)rows, 256, 0, s>>>(mask_key, p_.k, BodyPlanes40<1024>{hi, lo},
                                                                            pksk_.rows.get());
    HIP_CHECK(hipGetLastError());
    timer.mark(2);
    build_limbs(pksk_);
    timer.mark(3);
    HIP_CHECK(hipStreamSynchronize(s));
    timer.read(pk_load_ms_);
    key_guard.dismiss();
}

void Device::download_packing_key_compact(uint8_t* planes) {
    if (!has_packing_key()) throw Error(FR_ERR_INVALID, "no packing key on the device");
    need_pk_compact_point(p_, "device export of a compact packing key");
    const size_t rows = pk_rows(p_), N = (size_t)p_.N, bytes = pk_compact_planes(p_);
    const hipStream_t s = STREAM;
    gpu::DevBuf<uint8_t> d_planes(bytes);
    uint32_t* hi = reinterpret_cast<uint32_t*>(d_planes.get());
    uint8_t* lo = d_planes.get() + 4 * rows * N;
    if (N == 2048) k_gather_planes40<2048><<<(unsigned)rows, 256, 0, s>>>(p_.k, pksk_.rows.get(), hi, lo);
    else k_gather_planes40<1024><<<(unsigned)rows, 256, 0, s>>>(p_.k, pksk_.rows.get(), hi, lo);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(planes, d_planes.get(), bytes, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));  // the staging buffer goes once the copy has run
}

void Device::upload_packing_key(const void* rows) {
    Replacing key_guard([this] { drop_packing_key(); });
    pksk_.alloc_rows((int)pk_rows(p_), (int)pk_row_words(p_));
    HIP_CHECK(hipMemcpy(pksk_.rows.get(), rows, 8 * pk_len(p_), hipMemcpyHostToDevice));
    build_limbs(pksk_);
    HIP_CHECK(hipStreamSynchronize(cur().stream.get()));
    key_guard.dismiss();
}

void Device::download_packing_key(uint64_t* rows) {
    if (!has_packing_key()) throw Error(FR_ERR_INVALID, "no packing key on the device");
    HIP_CHECK(hipMemcpy(rows, pksk_.rows.get(), 8 * pksk_.rows.size(), hipMemcpyDeviceToHost));
}

void Device::download_server_key(uint64_t* ksk, size_t ksk_len, uint64_t* bsk, size_t bsk_len) {
    if (!ksk_ || !d_tbsk_) throw Error(FR_ERR_NO_KEY, "no device-generated server key");
    if (ksk) {
        if (ksk_len != ksk_.rows.size()) throw Error(FR_ERR_INVALID, "ksk size");
        HIP_CHECK(hipMemcpy(ksk, ksk_.rows.get(), 8 * ksk_len, hipMemcpyDeviceToHost));
    }
    if (bsk) {
        if (bsk_len != p_.bsk_len()) throw Error(FR_ERR_INVALID, "bsk size");
        HIP_CHECK(hipMemcpy(bsk, d_tbsk_.get(), 8 * bsk_len, hipMemcpyDeviceToHost));
    }
}

}  // namespace fr
