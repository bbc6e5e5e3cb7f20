// Linear combination of the input LWEs fused with the LWE keyswitch kN -> n (signed
// base 2^3, 5 levels) on MI355X (gfx950, CDNA4), and the Device methods that launch it.
//
//   k_lincomb_keyswitch : the VALU path (FR_KS_MFMA=0): lincomb + keyswitch in one kernel
//   k_ks_digits16, k_ks_digits : lincomb + gadget digits in MFMA fragment order
//   k_ks_mfma<MR,MC>    : digits x KSK byte limbs on v_mfma_i32_32x32x32_i8, MR row and
//                         MC column tiles per wave
//   k_ks_glds<SK,NB>    : the four-row-tile shape with both operands staged by LDS-DMA
//   k_ksk_limbs         : one-time KSK -> balanced byte limbs in fragment order
//   k_linear            : linear combination into a slot without a bootstrap
//   k_pack_rotate_sum   : the packing keyswitch's sum_j X^j G[j] (its digits and GEMM are the
//                         kernels above with the (2^7, 3) gadget and the packing key's limbs)
//   k_pack_compress     : the compact reply, every sent coefficient rounded to its top 16 bits
#include <algorithm>
#include <cstdlib>

#include "device_impl.h"
#include "keys.h"

namespace fr {

// ------------------------------------------------- lincomb + keyswitch
// Tile: 32 gates x 64 output columns x one slice of the kN input coefficients
// per 256-thread workgroup (split-K: the slices' partial sums are exact mod
// 2^64, so they are combined with 64-bit atomic adds into a zeroed output).
// Each wave owns 8 gates; each lane one output column.  Digits of the
// lincomb'd mask coefficients are staged in LDS per chunk of 32 coefficients;
// KSK rows are read once per tile, coalesced (64 consecutive u64 per wave).
constexpr int KS_BT = 32, KS_CT = 64, KS_CH = 32;

// arena slot of a gate input: s >= 0 is a slot; s < 0 a content reference of a
// template plan, resolved through the bound content map (Device::bind_content)
__device__ __forceinline__ int arena_slot(int s, const int* __restrict__ cmap) { return s >= 0 ? s : cmap[-1 - s]; }

template <int KSB, int KSL>
__global__ void __launch_bounds__(256)
k_lincomb_keyswitch(const DevGate* __restrict__ gates, int B, const uint64_t* __restrict__ arena, int slot_stride,
                    const int* __restrict__ cmap, const uint64_t* __restrict__ ksk, int n, int big,
                    int chunks_per_split, unsigned long long* __restrict__ out, int out_stride) {
    __shared__ int8_t dig[KS_BT][KS_CH][KSL];
    __shared__ DevGate sg[KS_BT];
    const int tid = threadIdx.x;
    const int col = blockIdx.y * KS_CT + (tid & 63);
    const int rg = tid >> 6;
    const int b0 = blockIdx.x * KS_BT;
    const int c_begin = blockIdx.z * chunks_per_split * KS_CH;
    const int c_end = min(big, c_begin + chunks_per_split * KS_CH);
    for (int e = tid; e < KS_BT; e += 256) {
        if (b0 + e < B) {
            sg[e] = gates[b0 + e];
            for (int q = 0; q < sg[e].n_in; ++q) sg[e].in_slot[q] = arena_slot(sg[e].in_slot[q], cmap);
        } else {
            sg[e].n_in = 0, sg[e].offset = 0;
        }
    }
    uint64_t acc[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) acc[r] = 0;
    for (int i0 = c_begin; i0 < c_end; i0 += KS_CH) {
        __syncthreads();
        for (int e = tid; e < KS_BT * KS_CH; e += 256) {
            const int row = e / KS_CH, ii = e % KS_CH;
            uint64_t v = 0;
            if (i0 + ii < c_end) {
                const DevGate& gg = sg[row];
                for (int q = 0; q < gg.n_in; ++q)
                    v += (uint64_t)(int64_t)gg.in_w[q] * arena[(size_t)gg.in_slot[q] * slot_stride + i0 + ii];
            }
            int32_t d[KSL];
            ks_decompose<KSB, KSL>(v, d);
#pragma unroll
            for (int j = 0; j < KSL; ++j) dig[row][ii][j] = (int8_t)d[j];
        }
        __syncthreads();
        if (col <= n) {
            const int lim = c_end - i0 < KS_CH ? c_end - i0 : KS_CH;
            for (int ii = 0; ii < lim; ++ii) {
#pragma unroll
                for (int j = 0; j < KSL; ++j) {
                    const uint64_t kv = ksk[((size_t)(i0 + ii) * KSL + j) * (n + 1) + col];
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        const int64_t d = dig[rg * 8 + r][ii][j];
                        acc[r] -= (uint64_t)d * kv;
                    }
                }
            }
        }
    }
    if (col <= n) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int row = rg * 8 + r, b = b0 + row;
            if (b >= B) continue;
            uint64_t v = acc[r];
            if (col == n && blockIdx.z == 0) {
                const DevGate& gg = sg[row];
                uint64_t body = (uint64_t)(int64_t)gg.offset << (DELTA_LOG - 1);
                for (int q = 0; q < gg.n_in; ++q)
                    body += (uint64_t)(int64_t)gg.in_w[q] * arena[(size_t)gg.in_slot[q] * slot_stride + big];
                v += body;
            }
            if (gridDim.z == 1) out[(size_t)b * out_stride + col] = v;
            else atomicAdd(&out[(size_t)b * out_stride + col], (unsigned long long)v);
        }
    }
}

// ------------------------------------------- keyswitch on int8 MFMA
// out[g][t] = [t == n] * body_g - sum_k D[g][k] * KSK[k][t]  (mod 2^64), with
// D the signed base-2^3 digits of the lincomb'd mask (|d| <= 4, k = 5i + level)
// and KSK split into 8 balanced byte limbs, KSK = sum_l L_l * 256^l (mod 2^64),
// L_l in [-128, 128).  Each sum_k D * L_l is an exact i32 GEMM (|.| <= 4 * 128 *
// 10240 < 2^31) on v_mfma_i32_32x32x32_i8; limbs recombine in the epilogue.
// Layouts: D (Bp rows: B rounded up to the wave's row tiles, zero rows) and L (limb
// column col*8 + l, padded with zero columns) in MFMA fragment order: the operand of
// (32-row tile, 32-k tile) is 1 KB contiguous, lane r + 32h holding row r, k = 16h..16h+15,
// so every fragment load of a wave is one fully coalesced 1 KB read.
typedef int v4i_t __attribute__((ext_vector_type(4)));
typedef int v16i_t __attribute__((ext_vector_type(16)));
// byte offset of (row, k) in a fragment-ordered operand with KT = KD / 32 k tiles
__device__ __forceinline__ size_t ks_frag(int row, int k, int KT) {
    return ((((size_t)(row >> 5) * KT + (k >> 5)) * 64 + (row & 31) + 32 * ((k >> 4) & 1)) << 4) + (k & 15);
}

// lincomb + digits: one thread per (gate, input coefficient); the body per gate.
// The same launch zeroes the mask words of each output row (the MFMA pass
// subtracts into them with atomics) and the padding digit rows B <= g < gridDim.y.
template <int KSB, int KSL>
__global__ void __launch_bounds__(256)
k_ks_digits(const DevGate* __restrict__ gates, int B, const uint64_t* __restrict__ arena, int slot_stride,
            const int* __restrict__ cmap, int big, int8_t* __restrict__ dig, uint64_t* __restrict__ ks, int ks_n,
            int ks_stride) {
    const int g = blockIdx.y, KT = big * KSL / 32;
    if (g >= B) {  // padding row of the last row tile: zero digits (16-byte halves of its fragments)
        for (int i = blockIdx.x * 256 + threadIdx.x; i < 2 * KT; i += gridDim.x * 256)
            *(int4*)(dig + ks_frag(g, 16 * i, KT)) = int4{0, 0, 0, 0};
        return;
    }
    const DevGate& gg = gates[g];
    const int nin = gg.n_in;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < ks_n; t += gridDim.x * 256) ks[(size_t)g * ks_stride + t] = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i <= big; i += gridDim.x * 256) {
        uint64_t v = i == big ? (uint64_t)(int64_t)gg.offset << (DELTA_LOG - 1) : 0;
        for (int q = 0; q < nin; ++q)
            v += (uint64_t)(int64_t)gg.in_w[q] * arena[(size_t)arena_slot(gg.in_slot[q], cmap) * slot_stride + i];
        if (i == big) {
            ks[(size_t)g * ks_stride + ks_n] = v;  // column n of the output row; the MFMA pass subtracts
        } else {
            int32_t d[KSL];
            ks_decompose<KSB, KSL>(v, d);
#pragma unroll
            for (int j = 0; j < KSL; ++j) dig[ks_frag(g, i * KSL + j, KT)] = (int8_t)d[j];
        }
    }
}

// The same pass, one workgroup per gate and sixteen consecutive coefficients per thread: its
// 16 KSL digits are KSL whole 16-byte pieces of the fragment-ordered digit row (k = 16 KSL q ..
// 16 KSL q + 16 KSL - 1 starts a piece), stored as 16-byte writes, where k_ks_digits's byte
// stores scatter every digit over 16-byte pieces of 10 fragments; the inputs load as 16-byte
// vectors.  (needs big % 16 == 0)  The inputs' slot lookups (content map included) and their
// body coefficients are fetched by one thread per input at once, and the mask loads of four
// inputs are in flight together: with one input at a time, a small level's fan-in-16 gates
// paid sixteen dependent memory round trips (≈19 µs per launch at 1-16 gates).
template <int KSB, int KSL>
__global__ void __launch_bounds__(128)
k_ks_digits16(const DevGate* __restrict__ gates, int B, const uint64_t* __restrict__ arena, int slot_stride,
              const int* __restrict__ cmap, int big, int8_t* __restrict__ dig, uint64_t* __restrict__ ks, int ks_n,
              int ks_stride) {
    const int g = blockIdx.x, KT = big * KSL / 32, groups = big / 16;
    if (g >= B) {  // padding row of the last row tile: zero digits
        for (int q = threadIdx.x; q < groups; q += blockDim.x)
#pragma unroll
            for (int c = 0; c < KSL; ++c) *(int4*)(dig + ks_frag(g, 16 * (q * KSL + c), KT)) = int4{0, 0, 0, 0};
        return;
    }
    __shared__ int slot_s[16];
    __shared__ uint64_t w_s[16], body_s[16];
    const DevGate& gg = gates[g];
    const int nin = gg.n_in;
    if (threadIdx.x < nin) {
        const int i = threadIdx.x;
        const int slot = arena_slot(gg.in_slot[i], cmap);
        const uint64_t w = (uint64_t)(int64_t)gg.in_w[i];
        slot_s[i] = slot;
        w_s[i] = w;
        body_s[i] = w * arena[(size_t)slot * slot_stride + big];
    }
    for (int t = threadIdx.x; t < ks_n; t += blockDim.x) ks[(size_t)g * ks_stride + t] = 0;
    __syncthreads();
    if (threadIdx.x == 0) {  // column n of the output row (the body); the MFMA pass subtracts
        uint64_t v = (uint64_t)(int64_t)gg.offset << (DELTA_LOG - 1);
        for (int q = 0; q < nin; ++q) v += body_s[q];
        ks[(size_t)g * ks_stride + ks_n] = v;
    }
    for (int q = threadIdx.x; q < groups; q += blockDim.x) {
        uint64_t v[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = 0;
        int qi = 0;
        for (; qi + 4 <= nin; qi += 4) {  // four inputs' loads in flight
            ulonglong2 x[4][8];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const ulonglong2* src = (const ulonglong2*)(arena + (size_t)slot_s[qi + u] * slot_stride + 16 * q);
#pragma unroll
                for (int e = 0; e < 8; ++e) x[u][e] = src[e];
            }
            __builtin_amdgcn_sched_barrier(0);  // keep the 32 loads ahead of their first use
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint64_t w = w_s[qi + u];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    v[2 * e] += w * x[u][e].x;
                    v[2 * e + 1] += w * x[u][e].y;
                }
            }
        }
        for (; qi < nin; ++qi) {
            const uint64_t w = w_s[qi];
            const ulonglong2* src = (const ulonglong2*)(arena + (size_t)slot_s[qi] * slot_stride + 16 * q);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const ulonglong2 x = src[e];
                v[2 * e] += w * x.x;
                v[2 * e + 1] += w * x.y;
            }
        }
        uint32_t words[4 * KSL];
#pragma unroll
        for (int b = 0; b < 4 * KSL; ++b) words[b] = 0;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            int32_t d[KSL];
            ks_decompose<KSB, KSL>(v[e], d);
#pragma unroll
            for (int j = 0; j < KSL; ++j) {
                const int byte = e * KSL + j;
                words[byte >> 2] |= (uint32_t)(uint8_t)(int8_t)d[j] << (8 * (byte & 3));
            }
        }
#pragma unroll
        for (int c = 0; c < KSL; ++c)
            *(uint4*)(dig + ks_frag(g, 16 * (q * KSL + c), KT)) =
                uint4{words[4 * c], words[4 * c + 1], words[4 * c + 2], words[4 * c + 3]};
    }
}

// one wave per MR x 1 tiles of 32 x 32 (gate, limb-column) and one K slice
// (z of GZ); 4 waves per workgroup along the column direction
// share the gate rows through L1, and the MR row tiles of a wave share each KSK
// fragment (MR-fold less KSK traffic).  Partial results are subtracted from out
// (pre-set to [t == n] * body) with 64-bit atomics: exact mod 2^64 in any order.
// Workgroup order (one-dimensional grid, XCD-aware).  The hardware deals workgroup b to
// XCD b % 8; XCD j takes the column groups [j GYX, (j+1) GYX) for every row group and
// K slice, so each KSK limb fragment is fetched into one XCD's L2 only, and the row
// groups of that XCD (dispatched next to each other: row group fastest) read it there.
// Without the remap, the row groups of a column group sat on different XCDs and each
// fetched the whole limb matrix (4x the KSK traffic at 512 gates).  xcd == 0: the plain
// order (row group fastest, then column group, then K slice) for A/B runs.
struct KsTile {
    int x, y, z;
};
__device__ __forceinline__ bool ks_tile(int b, int GX, int GY, int GZ, int xcd, KsTile& t) {
    if (!xcd) {
        t.x = b % GX, t.y = (b / GX) % GY, t.z = b / (GX * GY);
        return t.z < GZ;
    }
    const int GYX = (GY + 7) / 8, loc = b >> 3;
    t.x = loc % GX;
    t.z = (loc / GX) % GZ;
    t.y = (b & 7) * GYX + loc / (GX * GZ);
    return loc < GX * GZ * GYX && t.y < GY;
}
__host__ __device__ inline int ks_grid_blocks(int GX, int GY, int GZ, int xcd) {
    return xcd ? 8 * GX * GZ * ((GY + 7) / 8) : GX * GY * GZ;
}

// k-steps per stage of the LDS-DMA ring of k_ks_glds
#ifndef FR_KS_SK
#define FR_KS_SK 2
#endif
// stages in the LDS-DMA ring of k_ks_glds (NB - 1 in flight)
#ifndef FR_KS_NB
#define FR_KS_NB 4
#endif
// (k_ks_mfma: k-steps in flight per wave, 8 with one row tile, 2 with four; four with four
// row tiles took 512 gates from 100 to 158 us of keyswitch: the registers cost occupancy)
// limb l of KSK column t sits at limb column 8 t + l (the MFMA's column operand), so the 8
// limbs of a column land in 8 adjacent lanes of the accumulator.  (Measured and dropped in
// round 3: the limbs as the row operand, each lane recombining two whole columns in
// registers -- its atomics then scatter over 32 gate rows per instruction, 4x the memory-side
// atomic transactions: 512 gates 73 -> 83 us.)
__host__ __device__ inline int ks_limb_col(int t, int l) { return t * 8 + l; }
// one MFMA step of a wave: acc += (32 digit rows) x (32 limb columns), k = 32
__device__ __forceinline__ v16i_t ks_mma(v4i_t a, v4i_t b, v16i_t acc) {
    return __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc, 0, 0, 0);
}
// a 64-bit value from another lane of the row by a DPP move (dpp_ctrl CTRL, all rows and banks)
template <int CTRL>
__device__ __forceinline__ uint64_t ks_dpp64(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xF, 0xF, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xF, 0xF, false);
    return ((uint64_t)hi << 32) | lo;
}
// Epilogue: recombine the 8 byte limbs of each KSK column and subtract the wave's MR x MC
// tiles from out (pre-set to [t == n] * body) with 64-bit atomics (exact mod 2^64 in any
// order, so K slices meet there).  Rows g0 + 32 t, limb columns lcw + 32 c.
template <int MR, int MC>
__device__ __forceinline__ void ks_epilogue(const v16i_t (&acc)[MR][MC], int g0, int lcw, int r, int h, int B, int ncols,
                                            int nlc, unsigned long long* __restrict__ out, int out_stride) {
    // lane holds D[row][lc + r] for rows (i&3) + 8(i>>2) + 4h: limb l = r & 7 of
    // column (lc + r) / 8; the 8 limbs of a column meet across the lane's 8-lane group
    const int limb = r & 7;
#pragma unroll
    for (int c = 0; c < MC; ++c) {
        const int lc = lcw + 32 * c, col = (lc + r) >> 3;
        if (lc >= nlc) continue;  // uniform
#pragma unroll
        for (int t = 0; t < MR; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                uint64_t v = (uint64_t)(int64_t)acc[t][c][i] << (8 * limb);
                // sum over the 8 lanes of the column: DPP lane moves (quad_perm [1,0,3,2],
                // [2,3,0,1], then row_half_mirror pairs the two quads of each 8-lane group)
                v += ks_dpp64<0xB1>(v);
                v += ks_dpp64<0x4E>(v);
                v += ks_dpp64<0x141>(v);
                const int g = g0 + 32 * t + (i & 3) + 8 * (i >> 2) + 4 * h;
                if (limb == 0 && g < B && col < ncols && v != 0)
                    atomicAdd(&out[(size_t)g * out_stride + col], (unsigned long long)(0 - v));
            }
    }
}

template <int MR, int MC>
__global__ void __launch_bounds__(256)
k_ks_mfma(const int8_t* __restrict__ dig, const int8_t* __restrict__ kl, int B, int KD, int ncols /* n + 1 */,
          int nlc /* limb-columns, multiple of 32 */, unsigned long long* __restrict__ out, int out_stride, int GX,
          int GY, int GZ, int xcd) {
    constexpr int UN = MR * MC == 1 ? 8 : 2;  // k-steps in flight per wave
    KsTile tile;
    if (!ks_tile((int)blockIdx.x, GX, GY, GZ, xcd, tile)) return;  // padding workgroup (uniform)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int g0 = tile.x * 32 * MR;
    const int lcw = (tile.y * 4 + w) * 32 * MC;  // first limb-column of this wave's MC column tiles
    if (lcw >= nlc) return;  // whole wave
    const int kspan = KD / GZ, kb = tile.z * kspan, KT = KD / 32;
    // fragment (tile, k) at ((tile * KT + k / 32) * 64 + lane) * 16: one k step of 32 is 1 KB
    const int8_t* ap = dig + ((size_t)(g0 >> 5) * KT * 64 + lane) * 16 + (size_t)kb * 32;
    const int8_t* bp[MC];
#pragma unroll
    for (int c = 0; c < MC; ++c)  // a tile past the padded columns re-reads the last one (its result is dropped)
        bp[c] = kl + ((size_t)(min(lcw + 32 * c, nlc - 32) >> 5) * KT * 64 + lane) * 16 + (size_t)kb * 32;
    v16i_t acc[MR][MC];
#pragma unroll
    for (int t = 0; t < MR; ++t)
#pragma unroll
        for (int c = 0; c < MC; ++c) acc[t][c] = v16i_t{0};
    for (int k0 = 0; k0 < kspan; k0 += 32 * UN) {  // kspan is a multiple of 256 (host)
        v4i_t a[UN][MR], b[UN][MC];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
#pragma unroll
            for (int c = 0; c < MC; ++c) b[u][c] = *(const v4i_t*)(bp[c] + (size_t)(k0 + 32 * u) * 32);
#pragma unroll
            for (int t = 0; t < MR; ++t) a[u][t] = *(const v4i_t*)(ap + (size_t)t * KD * 32 + (size_t)(k0 + 32 * u) * 32);
        }
#pragma unroll
        for (int u = 0; u < UN; ++u)
#pragma unroll
            for (int t = 0; t < MR; ++t)
#pragma unroll
                for (int c = 0; c < MC; ++c)
                    acc[t][c] = ks_mma(a[u][t], b[u][c], acc[t][c]);
    }
    ks_epilogue<MR, MC>(acc, g0, lcw, r, h, B, ncols, nlc, out, out_stride);
}

// Four-row-tile keyswitch with both operands staged by LDS-DMA (global_load_lds, 16 B per
// lane, no VGPR staging) through a ring of NB stages of SK k-steps (round 3).  PMC at 512
// gates of a register-staged version (digit tiles shared through LDS): 70 % of wave cycles
// parked on memory waits, the MFMA pipes 16 % busy -- each wave kept only one or two k-steps
// of fragments in flight against the HBM / L2 latency (more registers for more in flight
// cost occupancy; sharing the digit tiles alone gained nothing).  Here
// NB - 1 stages are in flight per workgroup at no register cost.  Wave w moves row tile w
// of the digits and column tile w of the limbs; every wave reads the four digit tiles and
// its own limb tile from the stage.  One raw barrier per stage, a counted vmcnt (never 0
// in steady state) so the DMAs of later stages stay in flight across it.  512 / 254 gates:
// keyswitch 98-100 -> 89-90 / 62-64 -> 55-57 us (tools/ks_probe.py; SK 1 / NB 8, SK 2 /
// NB 5, SK 1 / NB 10 and 4, 8, 10 K slices all measured slower: profiles/r03/ab_ks_glds.log)
template <int N>
__device__ __forceinline__ void ks_wait_vm() {
    static_assert(N >= 0 && N < 64, "vmcnt range");
    // s_waitcnt simm16 (gfx9): vmcnt [3:0] + [15:14], expcnt [6:4] = 7, lgkmcnt [11:8] = 15 (no wait)
    __builtin_amdgcn_s_waitcnt((N & 15) | (((N >> 4) & 3) << 14) | (7 << 4) | (15 << 8));
}
// wait until at most `after` stages of L DMAs each remain in flight (after <= A)
template <int L, int A>
__device__ __forceinline__ void ks_wait_after(int after) {
    if constexpr (A > 0) {
        if (after >= A) {
            ks_wait_vm<A * L>();
            return;
        }
        ks_wait_after<L, A - 1>(after);
    } else {
        ks_wait_vm<0>();
    }
}
template <int SK, int NB>
__global__ void __launch_bounds__(256)
k_ks_glds(const int8_t* __restrict__ dig, const int8_t* __restrict__ kl, int B, int KD, int ncols, int nlc,
          unsigned long long* __restrict__ out, int out_stride, int GX, int GY, int GZ, int xcd) {
    constexpr int MR = 4, L = 2 * SK;  // DMAs per wave per stage
    static_assert(NB >= 2 && (NB - 2) * 2 * SK < 64, "ring depth");
    __shared__ v4i_t ring[NB][2][4][SK][64];  // [stage][digits, limbs][tile][k-step][lane]
    KsTile tile;
    if (!ks_tile((int)blockIdx.x, GX, GY, GZ, xcd, tile)) return;  // padding workgroup (uniform)
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int g0 = tile.x * 32 * MR;
    const int lcw = (tile.y * 4 + w) * 32;  // this wave's limb-column tile (past nlc: computed, dropped)
    const int kspan = KD / GZ, kb = tile.z * kspan, KT = KD / 32;
    const int8_t* ap = dig + ((size_t)((g0 >> 5) + w) * KT * 64 + lane) * 16 + (size_t)kb * 32;
    const int8_t* bp = kl + ((size_t)(min(lcw, nlc - 32) >> 5) * KT * 64 + lane) * 16 + (size_t)kb * 32;
    const int S = kspan / (32 * SK);  // kspan is a multiple of 256 (host)
    auto issue = [&](int st) {
        const int buf = st % NB;
#pragma unroll
        for (int u = 0; u < SK; ++u) {
            const size_t off = (size_t)(st * SK + u) * 32 * 32;
            __builtin_amdgcn_global_load_lds((const void*)(ap + off),
                                             (__attribute__((address_space(3))) void*)&ring[buf][0][w][u][0], 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const void*)(bp + off),
                                             (__attribute__((address_space(3))) void*)&ring[buf][1][w][u][0], 16, 0, 0);
        }
    };
    v16i_t acc[MR][1];
#pragma unroll
    for (int t = 0; t < MR; ++t) acc[t][0] = v16i_t{0};
#pragma unroll
    for (int st = 0; st < NB - 1; ++st)
        if (st < S) issue(st);
    for (int s = 0; s < S; ++s) {
        // this wave's DMAs of stage s have landed once at most those of the stages after it remain
        ks_wait_after<L, NB - 2>(min(NB - 2, S - 1 - s));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // every wave's stage s landed; stage s - 1's buffer read by all
        asm volatile("" ::: "memory");
        if (s + NB - 1 < S) issue(s + NB - 1);  // into stage s - 1's buffer
        const int cur = s % NB;
        v4i_t a[SK][MR], b[SK];
#pragma unroll
        for (int u = 0; u < SK; ++u) {
            b[u] = ring[cur][1][w][u][lane];
#pragma unroll
            for (int t = 0; t < MR; ++t) a[u][t] = ring[cur][0][t][u][lane];
        }
#pragma unroll
        for (int u = 0; u < SK; ++u)
#pragma unroll
            for (int t = 0; t < MR; ++t) acc[t][0] = ks_mma(a[u][t], b[u], acc[t][0]);
    }
    // Epilogue through LDS (the ring is free once every wave has passed the last stage): wave w
    // stores its 128 x 32 tile of i32 limb sums row-major ([row][limb column], 128 B rows,
    // conflict-free b32 stores), then lane L reads KSK column L & 3 of rows (L >> 2) + 16 j,
    // its 8 limbs as two b128 reads, recombines them in registers and subtracts the column with
    // one atomic: 8 atomics per lane, 16 rows x 4 adjacent columns per instruction (against 64
    // values x three 64-bit DPP rounds per lane in ks_epilogue)
    __syncthreads();
    if (lcw >= nlc) return;  // whole wave (no barrier below)
    int* tl = (int*)&ring[0][0][0][0][0] + w * 128 * 32;
#pragma unroll
    for (int t = 0; t < MR; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) tl[(32 * t + (i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r] = acc[t][0][i];
    const int c = lane & 3, col = (lcw >> 3) + c;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int row = (lane >> 2) + 16 * j, g = g0 + row;
        const v4i_t lo = *(const v4i_t*)(tl + row * 32 + 8 * c), hi = *(const v4i_t*)(tl + row * 32 + 8 * c + 4);
        uint64_t v = 0;
#pragma unroll
        for (int l = 0; l < 4; ++l) v += ((uint64_t)(int64_t)lo[l] << (8 * l)) + ((uint64_t)(int64_t)hi[l] << (8 * l + 32));
        if (g < B && col < ncols && v != 0) atomicAdd(&out[(size_t)g * out_stride + col], (unsigned long long)(0 - v));
    }
}

// KSK (u64 [k][t], t <= n) -> balanced byte limbs in fragment order, limb l of column t at
// limb column ks_limb_col(t, l)
__global__ void __launch_bounds__(256) k_ksk_limbs(const uint64_t* __restrict__ ksk, int KD, int ncols, int nlc,
                                                   int8_t* __restrict__ kl) {
    const int KT = KD / 32;
    const int k = blockIdx.x * 256 + threadIdx.x;
    const int t = blockIdx.y;
    if (k >= KD) return;
    uint64_t x = t < ncols ? ksk[(size_t)k * ncols + t] : 0;
#pragma unroll
    for (int l = 0; l < 8; ++l) {
        int v = (int)(x & 255);
        x >>= 8;
        if (v >= 128) {
            v -= 256;
            x += 1;
        }
        const int lc = ks_limb_col(t, l);
        if (lc < nlc) kl[ks_frag(lc, k, KT)] = (int8_t)v;
    }
}

// linear combination into a slot (no bootstrap): NOT of a boolean, a match's final
// affine map.  The gate travels as a kernel argument (no staging copy before the launch).
__global__ void __launch_bounds__(256) k_linear(const DevGate gg, uint64_t* __restrict__ arena, int slot_stride,
                                                int len) {
    uint64_t* out = arena + (size_t)gg.out_slot[0] * slot_stride;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < len; t += gridDim.x * 256) {
        uint64_t v = (t == len - 1) ? ((uint64_t)(int64_t)gg.offset << (DELTA_LOG - 1)) : 0;
        for (int q = 0; q < gg.n_in; ++q) v += (uint64_t)(int64_t)gg.in_w[q] * arena[(size_t)gg.in_slot[q] * slot_stride + t];
        out[t] = v;
    }
}

// ================================================================== host side
void Device::init_ks() {
    if (const char* ev = std::getenv("FR_KS_MFMA")) ks_mfma_ = std::atoi(ev) != 0;
    if (const char* ev = std::getenv("FR_KS_MR4_MIN")) ks_mr4_min_ = (size_t)std::atol(ev);
    if (const char* ev = std::getenv("FR_KS_MC")) ks_mc_ = std::atoi(ev);
    if (const char* ev = std::getenv("FR_KS_SPLIT")) ks_split_ = std::atoi(ev);
    if (const char* ev = std::getenv("FR_KS_XCD")) ks_xcd_ = std::atoi(ev) != 0;
    if (const char* ev = std::getenv("FR_KS_LDS")) ks_lds_ = std::atoi(ev) != 0;
    if (const char* ev = std::getenv("FR_KS_DIG16")) ks_dig16_ = std::atoi(ev) != 0;
    if (const char* ev = std::getenv("FR_PK_SPLIT")) pk_split_ = std::atoi(ev);
}

void Device::ensure_digits(size_t rows) {
    const size_t row = (size_t)p_.big() * p_.ks_level;
    if (rows * row <= cur().dig.size()) return;
    HIP_CHECK(hipStreamSynchronize(STREAM));
    cur().dig.grow(rows * row, 1024 * row);
}

// byte-limb form of a key's torus rows, the MFMA keyswitch's column operand
void Device::build_limbs(LimbKey& key) {
    const size_t bytes = (size_t)key.nlc * key.KD;
    key.limbs.alloc(bytes);
    HIP_CHECK(hipMemsetAsync(key.limbs.get(), 0, bytes, STREAM));
    k_ksk_limbs<<<dim3((unsigned)((key.KD + 255) / 256), (unsigned)(key.nlc / 8)), 256, 0, STREAM>>>(
        key.rows.get(), key.KD, key.ncols, key.nlc, key.limbs.get());
    HIP_CHECK(hipGetLastError());
}

// lincomb + digits of `padded` rows.  The byte-store pass (FR_KS_DIG16=0, or kN no multiple of
// 16) is compiled for the LWE gadget only; the packing keyswitch always takes k_ks_digits16.
template <int KSB, int KSL>
void Device::launch_ks_digits(const DevGate* d_gates, size_t n, size_t padded, int8_t* dig, uint64_t* out, int out_n,
                              int out_stride, hipEvent_t ev_start) {
    auto launch = [&](auto kernel, dim3 grid, int threads) {
        hipExtLaunchKernelGGL(kernel, grid, dim3(threads), 0, STREAM, ev_start, nullptr, 0, d_gates, (int)n,
                              (const uint64_t*)d_arena_.get(), p_.slot_stride(), (const int*)cur().cmap.device(), p_.big(),
                              dig, out, out_n, out_stride);
        HIP_CHECK(hipGetLastError());
    };
    if constexpr (KSB == 3 && KSL == 5)
        if (!ks_dig16_ || p_.big() % 16) return launch(k_ks_digits<KSB, KSL>, dim3(8, (unsigned)padded), 256);
    launch(k_ks_digits16<KSB, KSL>, dim3((unsigned)padded), 128);
}

// out -= dig x key.limbs: every MFMA kernel takes the same arguments, the shape picks one
void Device::launch_limb_gemm(const int8_t* dig, const LimbKey& key, size_t n, const KsShape& sh, uint64_t* out,
                              int out_stride, hipEvent_t ev_stop) {
    const int GX = (int)(sh.padded / (32 * sh.MR)), GY = (key.nlc + 128 * sh.MC - 1) / (128 * sh.MC);
    auto launch = [&](auto kernel) {
        hipExtLaunchKernelGGL(kernel, dim3((unsigned)ks_grid_blocks(GX, GY, sh.GZ, ks_xcd_)), dim3(256), 0, STREAM, nullptr,
                              ev_stop, 0, dig, (const int8_t*)key.limbs.get(), (int)n, key.KD, key.ncols, key.nlc,
                              (unsigned long long*)out, out_stride, GX, GY, sh.GZ, ks_xcd_);
        HIP_CHECK(hipGetLastError());
    };
    if (sh.MR == 4 && sh.MC == 1 && sh.lds) launch(k_ks_glds<FR_KS_SK, FR_KS_NB>);
    else if (sh.MR == 4 && sh.MC == 2) launch(k_ks_mfma<4, 2>);
    else if (sh.MR == 4) launch(k_ks_mfma<4, 1>);
    else launch(k_ks_mfma<1, 1>);
}

void Device::launch_ks(const DevGate* d_gates, size_t n, uint64_t* d_ks, hipEvent_t e0, hipEvent_t e1) {
    if (ks_mfma_) {
        const int KD = p_.big() * p_.ks_level;
        if (KD % 256) throw Error(FR_ERR_INVALID, "MFMA keyswitch needs kN*ks_level % 256 == 0");
        KsShape sh = ks_shape(n);
        ensure_digits(sh.padded);
        int8_t* d_dig = cur().dig.get();
        launch_ks_digits<3, 5>(d_gates, n, sh.padded, d_dig, d_ks, p_.n, p_.ks_stride(), e0);
        // column tiles per wave: 1 (FR_KS_MC=2 shares each digit fragment between two; with
        // fragment-ordered operands that no longer pays: 512 gates 121 -> 103 us at 1)
        sh.MC = sh.MR == 4 && ks_mc_ == 2 ? 2 : 1;
        sh.lds = ks_lds_;
        // K slices (partial sums meet in 64-bit atomics, so more slices cost atomic traffic, and
        // every slice its epilogue): 8 for one row tile per wave (1-17 gates ~30 us); four row
        // tiles (k_ks_glds): 5 up to 256 gates, 2 up to 512, then 1 (profiles/r03/ab_ks_glds.log:
        // 254 gates 55 us at 4-5 against 60 at 2; 512: 77 at 2 against 86-89 at 4-5; 1024 /
        // 2048: 125 / 231 at 1 against 130 / 234 at 2); a divisor of KD / 256
        const int gx = (int)(sh.padded / (32 * sh.MR));
        sh.GZ = sh.MR == 1 ? 8 : gx <= 2 ? 5 : gx <= 4 ? 2 : 1;
        while ((KD / 256) % sh.GZ) --sh.GZ;
        if (ks_split_ > 0 && (KD / 256) % ks_split_ == 0) sh.GZ = ks_split_;
        launch_limb_gemm(d_dig, ksk_, n, sh, d_ks, p_.ks_stride(), e1);
        return;
    }
    const uint64_t* arena = d_arena_.get();
    const int* d_cmap = cur().cmap.device();
    const int btiles = (int)((n + KS_BT - 1) / KS_BT);
    const int ctiles = (p_.n + 1 + KS_CT - 1) / KS_CT;
    const int chunks = (p_.big() + KS_CH - 1) / KS_CH;
    // enough workgroups to fill 256 CUs several times over, in whole chunks
    int splits = (2048 + btiles * ctiles - 1) / (btiles * ctiles);
    splits = std::max(1, std::min(splits, chunks));
    const int per = (chunks + splits - 1) / splits;
    splits = (chunks + per - 1) / per;
    if (splits > 1) HIP_CHECK(hipMemsetAsync(d_ks, 0, (size_t)8 * p_.ks_stride() * n, STREAM));
    dim3 grid((unsigned)btiles, (unsigned)ctiles, (unsigned)splits);
    hipExtLaunchKernelGGL(k_lincomb_keyswitch<3, 5>, grid, dim3(256), 0, STREAM, e0, e1, 0, d_gates, (int)n,
                          arena, p_.slot_stride(), d_cmap, (const uint64_t*)ksk_.rows.get(), p_.n,
                          p_.big(), per, (unsigned long long*)d_ks, p_.ks_stride());
    HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------- packing keyswitch
// n <= N booleans into the N coefficients of one GLWE under the client's key (keys.h):
//   G[j] = (0, .., 0, b_j) - D[j] x PKSK     the keyswitch above with the (2^7, 3) gadget, KD = 3 kN
//                                            rows of (k+1) N columns; b_j at column kN
//   out  = sum_j X^j G[j]                    k_pack_rotate_sum
// The digit and MFMA kernels are the LWE keyswitch's, with this operand's KD, columns and stride.

// out[c][t] += sum_{j0 <= j < j1} +-G[j][c][(t - j) mod N], negated where t < j (X^N = -1).  One
// thread per output word and j slice (blockIdx.y); for a fixed j a wave reads 64 consecutive
// words (two runs at the wrap).  The slices meet in 64-bit atomics, exact mod 2^64 in any
// order, in an output zeroed before.  W = (k+1) N is a multiple of 256, N a power of two.
__global__ void __launch_bounds__(256) k_pack_rotate_sum(const uint64_t* __restrict__ G, int n, int N, int W, int jper,
                                                         unsigned long long* __restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    const int t = c & (N - 1), base = c - t;
    const int j0 = blockIdx.y * jper, j1 = min(n, j0 + jper);
    uint64_t acc = 0;
    for (int j = j0; j < j1; ++j) {
        const int d = t - j;
        const uint64_t v = G[(size_t)j * W + base + (d >= 0 ? d : d + N)];
        acc = d >= 0 ? acc + v : acc - v;
    }
    if (c < W && acc != 0) atomicAdd(&out[c], (unsigned long long)acc);
}

// The same sum where start j reads row map[j] (a scan's window classes: several starts share a
// row): out[c][t] += sum_{j0 <= j < j1, map[j] >= 0} +-G[map[j]][c][(t - j) mod N].  The geometry
// is k_pack_rotate_sum's.  j comes from blockIdx and the loop counter alone, so map[j] is the same
// in every lane: one scalar load per start, a branch the whole wave takes or skips, and for a
// fixed j still 64 consecutive words of one row.  Every entry is < the row count (check_pack_map).
__global__ void __launch_bounds__(256) k_pack_map_sum(const uint64_t* __restrict__ G, const int* __restrict__ map, int n,
                                                      int N, int W, int jper, unsigned long long* __restrict__ out) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    const int t = c & (N - 1), base = c - t;
    const int j0 = blockIdx.y * jper, j1 = min(n, j0 + jper);
    uint64_t acc = 0;
    for (int j = j0; j < j1; ++j) {
        const int r = map[j];
        if (r < 0) continue;
        const int d = t - j;
        const uint64_t v = G[(size_t)r * W + base + (d >= 0 ? d : d + N)];
        acc = d >= 0 ? acc + v : acc - v;
    }
    if (c < W && acc != 0) atomicAdd(&out[c], (unsigned long long)acc);
}

// The compact reply (keys.h: packed_round16): out[c] = ((in[c] + 2^47) >> 48) mod 2^16 for the
// total = kN + n coefficients the blob carries; the body's first n follow the masks in the words
// as they do in the blob, so input and output share the index.  A separate launch: the
// rotate-sum's slices meet in atomics, so no thread of it sees a finished word.  Thread i rounds
// the eight coefficients from min(8 i, total - 8) and issues one 16-byte store.  The last thread's
// eight end at `total`, so nothing is written past it; where total is no multiple of 8 they
// overlap the thread before's, which stores the same values, and that one store is only 2-byte
// aligned (a global store need not be aligned).  total >= kN >= 8.
typedef unsigned short v8u16_t __attribute__((ext_vector_type(8)));
typedef v8u16_t v8u16_unaligned_t __attribute__((aligned(2)));
__global__ void __launch_bounds__(256) k_pack_compress(const uint64_t* __restrict__ in, int total,
                                                       uint16_t* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (8 * i >= total) return;
    const int s = min(8 * i, total - 8);
    v8u16_t v;
#pragma unroll
    for (int u = 0; u < 8; ++u)
        v[u] = (unsigned short)((in[s + u] + ((uint64_t)1 << (PKCRES_DROP - 1))) >> PKCRES_DROP);  // packed_round16
    *(v8u16_unaligned_t*)(out + s) = v;
}

// test hook: column t of a limb operand put back together, out[k] = sum_l L_l[k] 256^l (mod 2^64)
__global__ void __launch_bounds__(256) k_limb_column(const int8_t* __restrict__ kl, int KD, int t,
                                                     uint64_t* __restrict__ out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= KD) return;
    uint64_t v = 0;
#pragma unroll
    for (int l = 0; l < 8; ++l) v += (uint64_t)(int64_t)kl[ks_frag(ks_limb_col(t, l), k, KD / 32)] << (8 * l);
    out[k] = v;
}

void Device::packing_limb_column(int col, uint64_t* out_host) {
    if (!has_packing_key()) throw Error(FR_ERR_INVALID, "no packing key on the device");
    const int KD = pksk_.KD;
    if (col < 0 || col >= pksk_.ncols) throw Error(FR_ERR_INVALID, "packing key: column out of range");
    gpu::DevBuf<uint64_t> d((size_t)KD);
    k_limb_column<<<(KD + 255) / 256, 256, 0, STREAM>>>(pksk_.limbs.get(), KD, col, d.get());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out_host, d.get(), 8 * (size_t)KD, hipMemcpyDeviceToHost, STREAM));
    HIP_CHECK(hipStreamSynchronize(STREAM));
}

void Device::pack_bools(const DevGate* gates, size_t n, uint64_t* out_host) {
    pack_launch(gates, n, nullptr, n, out_host, nullptr);
}
void Device::pack_bools_compact(const DevGate* gates, size_t n, uint16_t* out_host) {
    pack_launch(gates, n, nullptr, n, nullptr, out_host);
}
void Device::pack_mapped(const DevGate* rows, size_t R, const int32_t* map, size_t n, uint64_t* out_words,
                         uint16_t* out_c16) {
    if (!map || !out_words == !out_c16) throw Error(FR_ERR_INVALID, "mapped pack: a map and one output form");
    check_pack_map(map, n, R, (size_t)p_.N);  // before anything is staged
    pack_launch(rows, R, map, n, out_words, out_c16);
}

// R rows through the digits and the GEMM, then n starts: start j reads row map[j] (map NULL:
// row j, R == n)
void Device::pack_launch(const DevGate* gates, size_t R, const int32_t* map, size_t n, uint64_t* out_words,
                         uint16_t* out_c16) {
    if (!has_packing_key()) throw Error(FR_ERR_INVALID, "no packing key on the device");
    const int N = p_.N, big = p_.big(), KD = pksk_.KD, W = pksk_.ncols;
    if (n < 1 || n > (size_t)N) throw Error(FR_ERR_INVALID, "pack: 1 <= n <= N booleans");
    if (KD % 256 || big % 16 || W % 256) throw Error(FR_ERR_INVALID, "pack: kN must be a multiple of 256");
    for (size_t j = 0; j < R; ++j) {
        const DevGate& g = gates[j];
        if (g.n_in < 0 || g.n_in > 16) throw Error(FR_ERR_INVALID, "pack: bad descriptor");
        for (int q = 0; q < g.n_in; ++q)
            if (g.in_slot[q] < 0 || (size_t)g.in_slot[q] >= next_slot_) throw Error(FR_ERR_INVALID, "pack: bad input slot");
    }
    const hipStream_t s = STREAM;
    LaneState& l = cur();
    KsShape sh = ks_shape(R);  // (one column tile and the LDS-DMA ring, whatever FR_KS_MC / FR_KS_LDS say)
    const size_t bp = sh.padded;  // rows of whole tiles, as launch_ks
    // scratch: the descriptors, digits [bp][KD], G [R][W] and the packed GLWE behind it, and the compact form's
    // W rounded values (kN + n <= W of them used); allocated at the first pack of the lane, doubled from there
    if (bp * KD > l.pk_dig.size() || (R + 1) * (size_t)W > l.pk_g.size() || R > l.pk_gates.size() || !l.pk_c16) {
        HIP_CHECK(hipStreamSynchronize(s));
        l.pk_dig.grow(bp * KD, (size_t)128 * KD);
        l.pk_g.grow((R + 1) * (size_t)W, (size_t)129 * W);
        l.pk_gates.grow(R, 128);
        l.pk_c16.grow((size_t)W, (size_t)W);
    }
    if (map && !l.pk_map) l.pk_map.alloc((size_t)N);  // n <= N entries
    int8_t* d_dig = l.pk_dig.get();
    uint64_t* d_g = l.pk_g.get();
    uint64_t* d_out = d_g + R * (size_t)W;
    DevGate* d_gates = l.pk_gates.get();
    HIP_CHECK(hipMemcpyAsync(d_gates, gates, sizeof(DevGate) * R, hipMemcpyHostToDevice, s));
    if (map) HIP_CHECK(hipMemcpyAsync(l.pk_map.get(), map, sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
    StageTimer<4> timer(profiling_ != 0, s);
    // the digit pass zeroes the mask columns of G and writes column kN: the rest of the body
    // polynomial's columns (from kN, ahead of that write) and the output row are zeroed here,
    // inside the first stage's time
    timer.mark(0);
    HIP_CHECK(hipMemset2DAsync(d_g + big, 8 * (size_t)W, 0, 8 * (size_t)N, R, s));
    HIP_CHECK(hipMemsetAsync(d_out, 0, 8 * (size_t)W, s));
    launch_ks_digits<PK_BASE_LOG, PK_LEVELS>(d_gates, R, bp, d_dig, d_g, big, W, nullptr);
    timer.mark(1);
    // Tiles for 32768 limb columns: GY = 256 column groups (the LWE keyswitch has 47) fill the
    // 256 CUs without K slices, so the four-row-tile shape runs unsliced (tools/pack_probe.py,
    // profiles/packed_results: 256 rows 68 us at 1 slice, 78 at 2, 117 at 8; 2048 rows 485 /
    // 540 / 939) and one row tile per wave takes 2 (16 rows: 33 us at 2 and 4, 38 at 1)
    sh.GZ = sh.MR == 1 ? 2 : 1;  // a divisor of KD / 256 = 24
    if (pk_split_ > 0 && (KD / 256) % pk_split_ == 0) sh.GZ = pk_split_;
    launch_limb_gemm(d_dig, pksk_, R, sh, d_g, W, nullptr);
    timer.mark(2);
    const int jper = 32, slices = (int)((n + jper - 1) / jper);
    const dim3 grid((unsigned)(W / 256), (unsigned)slices);
    if (map) k_pack_map_sum<<<grid, 256, 0, s>>>(d_g, l.pk_map.get(), (int)n, N, W, jper, (unsigned long long*)d_out);
    else k_pack_rotate_sum<<<grid, 256, 0, s>>>(d_g, (int)n, N, W, jper, (unsigned long long*)d_out);
    HIP_CHECK(hipGetLastError());
    timer.mark(3);
    if (out_c16) {
        const int total = big + (int)n;  // <= W, the size of pk_c16
        k_pack_compress<<<(unsigned)((total + 2047) / 2048), 256, 0, s>>>(d_out, total, l.pk_c16.get());
        HIP_CHECK(hipGetLastError());
        timer.mark(4);
        HIP_CHECK(hipMemcpyAsync(out_c16, l.pk_c16.get(), 2 * (size_t)total, hipMemcpyDeviceToHost, s));
    } else {
        timer.mark(4);
        HIP_CHECK(hipMemcpyAsync(out_words, d_out, 8 * (size_t)W, hipMemcpyDeviceToHost, s));
    }
    HIP_CHECK(hipStreamSynchronize(s));
    timer.read(pack_ms_);
}

void Device::run_linear(const DevGate& g) {
    k_linear<<<(p_.lwe_len() + 255) / 256, 256, 0, STREAM>>>(g, d_arena_.get(), p_.slot_stride(), p_.lwe_len());
    HIP_CHECK(hipGetLastError());
}

}  // namespace fr
