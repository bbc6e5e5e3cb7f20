// Private search over clear content (FFT ring): sample extracts of selectors at known
// coefficients, summed per gate.
//
//   k_select_sum : one workgroup per sum.  A selector is a GLWE ciphertext (A_0 .. A_{k-1}, B) whose
//                  phase is the direct test polynomial of a 16-bit table; for a content nibble v the
//                  table's bit v sits at coefficient j = v N/16, and the sample extract at j under
//                  the flattened key is
//                      out[c N + t] = t <= j ? A_c[j - t] : -A_c[N + j - t],    out[k N] = B[j].
//                  The kernel adds the extracts of a sum's <= 16 terms word by word (wrapping u64,
//                  exact) and writes the one big LWE into the sum's arena slot: no LWE per term
//                  ever exists.  Lane l of a pass writes word t = base + l and reads coefficient
//                  (j - t) mod N of each term's polynomial, so a wave's reads are one run of 64
//                  consecutive words taken backwards (two runs where t passes j), as coalesced as
//                  its stores.  The table (at most 128 selectors, 4 MB) stays in L2; the writes go
//                  to HBM.
//                  BYTES (a byte-table needle): term (i, pos, 0) reads table i of 256 entries, N/256
//                  of them to a selector, whose bit b sits at coefficient j = (i % (N/256)) 256 + b
//                  of selector i / (N/256) with no box around it, so every j of [0, N) occurs.  The
//                  extraction formula, the access shape and everything after the two index words are
//                  the same body; only the setup differs.
#include <cstring>

#include "device_impl.h"

namespace fr {

template <int N, int K, bool BYTES>
__global__ void __launch_bounds__(256) k_select_sum(const uint64_t* __restrict__ table, const uint8_t* __restrict__ text,
                                                    const DevSum* __restrict__ sums, uint64_t* __restrict__ arena,
                                                    int stride) {
    constexpr int W = (K + 1) * N, PASSES = K * N / 256;
    static_assert(K * N % 256 == 0 && N % 256 == 0, "a pass of 256 words stays inside one polynomial");
    __shared__ int s_base[SUM_MAX_TERMS];  // word offset of the term's selector in the table
    __shared__ int s_j[SUM_MAX_TERMS];     // the coefficient extracted
    const DevSum& S = sums[blockIdx.x];
    const int nt = S.n_terms;
    if ((int)threadIdx.x < nt) {
        const int q = S.term[threadIdx.x][0], pos = S.term[threadIdx.x][1], h = S.term[threadIdx.x][2];
        if constexpr (BYTES) {
            constexpr int TPG = N / 256;  // tables per selector
            (void)h;
            s_base[threadIdx.x] = (q / TPG) * W;
            s_j[threadIdx.x] = (q % TPG) * 256 + (int)text[pos];
        } else {
            s_base[threadIdx.x] = q * W;
            s_j[threadIdx.x] = (int)((text[pos] >> (4 * h)) & 15) * (N / 16);
        }
    }
    __syncthreads();
    uint64_t acc[PASSES];
    FR_UNROLL
    for (int r = 0; r < PASSES; ++r) acc[r] = 0;
    for (int i = 0; i < nt; ++i) {
        const uint64_t* sel = table + s_base[i];
        const int j = s_j[i];
        FR_UNROLL
        for (int r = 0; r < PASSES; ++r) {
            const int w = r * 256 + (int)threadIdx.x, c = w / N, d = j - (w % N);
            const uint64_t v = sel[c * N + (d & (N - 1))];
            acc[r] += d >= 0 ? v : 0 - v;
        }
    }
    uint64_t* out = arena + (size_t)S.out_slot * stride;
    FR_UNROLL
    for (int r = 0; r < PASSES; ++r) out[r * 256 + threadIdx.x] = acc[r];
    if (threadIdx.x == 0) {
        uint64_t b = 0;
        for (int i = 0; i < nt; ++i) b += table[s_base[i] + K * N + s_j[i]];
        out[K * N] = b;
    }
}

void Device::validate_sums(const DevSum* sums, size_t n, size_t n_sel, size_t text_n, NeedleForm form) const {
    for (size_t i = 0; i < n; ++i) {
        const DevSum& s = sums[i];
        if (s.n_terms < 1 || s.n_terms > SUM_MAX_TERMS) throw Error(FR_ERR_INVALID, "extract-sum: 1 <= n_terms <= 16");
        if (s.out_slot < 0 || (size_t)s.out_slot >= next_slot_) throw Error(FR_ERR_INVALID, "extract-sum: bad output slot");
        for (int t = 0; t < s.n_terms; ++t) {
            if (s.term[t][0] < 0 || (size_t)s.term[t][0] >= n_sel)
                throw Error(FR_ERR_INVALID, "extract-sum: selector index past the selector table bound");
            if (s.term[t][1] < 0 || (size_t)s.term[t][1] >= text_n)
                throw Error(FR_ERR_INVALID, "extract-sum: content position past the content bound");
            if (s.term[t][2] < 0 || s.term[t][2] > 1) throw Error(FR_ERR_INVALID, "extract-sum: half is 0 or 1");
            // (a byte table's index was checked against m above: n_sel is the tables bound)
            if (form == NEEDLE_BYTES && s.term[t][2] != 0)
                throw Error(FR_ERR_INVALID, "extract-sum: a byte table has no half");
        }
    }
}

void Device::bind_text(const uint8_t* text, size_t n) {
    LaneState& l = cur();
    l.text_n = 0;  // (an error below leaves no content bound)
    if (!n) return;
    if (!text) throw Error(FR_ERR_INVALID, "content bytes missing");
    const hipStream_t s = STREAM;
    l.text.reserve(n, 4096, s);  // (after a reallocation no launch reads the old bytes)
    std::memcpy(l.text.acquire(), text, n);
    l.text.commit(n, s);
    l.text_n = n;
}

void Device::launch_select_sum(const uint64_t* table, const DevSum* d_sums, size_t n) {
    const hipStream_t s = STREAM;
    const uint8_t* text = cur().text.device();
    const bool bytes = cur().sel_form == NEEDLE_BYTES;  // the bound needle's form picks the variant
    const auto launch = [&](auto kernel) {
        kernel<<<(unsigned)n, 256, 0, s>>>(table, text, d_sums, d_arena_.get(), p_.slot_stride());
    };
    if (p_.k == 1 && p_.N == 2048)
        bytes ? launch(k_select_sum<2048, 1, true>) : launch(k_select_sum<2048, 1, false>);
    else if (p_.k == 2 && p_.N == 1024)
        bytes ? launch(k_select_sum<1024, 2, true>) : launch(k_select_sum<1024, 2, false>);
    else
        throw Error(FR_ERR_INVALID, "extract-sum: (k, N) not compiled");
    HIP_CHECK(hipGetLastError());
}

void Device::check_sums(const DevSum* host, size_t n) const {
    if (p_.ring != FR_RING_FFT) throw Error(FR_ERR_INVALID, "private search: FFT ring only");
    if (n > (size_t)1 << 24) throw Error(FR_ERR_INVALID, "extract-sum: more than 2^24 sums");
    if (!cur().sel) throw Error(FR_ERR_INVALID, "extract-sum: no selector table bound");
    validate_sums(host, n, cur().sel_n, cur().text_n, cur().sel_form);
}

void Device::run_sums(const DevSum* sums, size_t n) {
    if (!n) return;
    if (lane_ != 0) throw Error(FR_ERR_INVALID, "staged extract-sums run on lane 0 only");
    check_sums(sums, n);
    const hipStream_t s = STREAM;
    sums_.reserve(n, 1024, s);
    std::memcpy(sums_.acquire(), sums, sizeof(DevSum) * n);
    sums_.commit(n, s);
    launch_select_sum(cur().sel, sums_.device(), n);
}

void Device::run_sums_resident(const DevSum* d_sums, const DevSum* host, size_t n) {
    if (!n) return;
    check_sums(host, n);
    launch_select_sum(cur().sel, d_sums, n);
}

gpu::DevBuf<DevSum> Device::upload_sums(const DevSum* sums, size_t n) {
    validate_sums(sums, n, (size_t)MAX_SELECTORS, (size_t)1 << 24);
    gpu::DevBuf<DevSum> d(std::max<size_t>(n, 1));
    HIP_CHECK(hipMemcpy(d.get(), sums, sizeof(DevSum) * n, hipMemcpyHostToDevice));
    return d;
}

void Device::select_sum_host(const DevNeedle& needle, const uint8_t* text, size_t len, const int32_t* terms,
                             const int32_t* n_terms, size_t n, uint64_t* out) {
    if (p_.ring != FR_RING_FFT) throw Error(FR_ERR_INVALID, "private search: FFT ring only");
    if (lane_ != 0) throw Error(FR_ERR_INVALID, "parity hooks run on lane 0 only");
    if (needle.dev != this || !needle.words) throw Error(FR_ERR_INVALID, "needle: uploaded to another context");
    if (!n) return;
    if (n > (size_t)1 << 16) throw Error(FR_ERR_INVALID, "extract-sum hook: at most 2^16 sums");
    std::vector<DevSum> sums(n);
    Slots slots(*this, n);
    for (size_t i = 0, at = 0; i < n; ++i) {
        DevSum& s = sums[i];
        std::memset(&s, 0, sizeof s);
        if (n_terms[i] < 1 || n_terms[i] > SUM_MAX_TERMS) throw Error(FR_ERR_INVALID, "extract-sum: 1 <= n_terms <= 16");
        s.n_terms = n_terms[i];
        s.out_slot = slots[i];
        std::memcpy(s.term, terms + 3 * at, sizeof(int32_t) * 3 * (size_t)s.n_terms);
        at += (size_t)s.n_terms;
    }
    const uint64_t* prev = cur().sel;
    const size_t prev_n = cur().sel_n;
    const NeedleForm prev_form = cur().sel_form;
    bind_selectors(needle.words.get(), needle.tables(), needle.form);
    try {
        bind_text(text, len);
        check_sums(sums.data(), n);  // before anything is staged or launched
        StageTimer<1> timer(profiling_ != 0, STREAM);
        const hipStream_t s = STREAM;
        sums_.reserve(n, 1024, s);
        std::memcpy(sums_.acquire(), sums.data(), sizeof(DevSum) * n);
        sums_.commit(n, s);
        timer.mark(0);
        launch_select_sum(cur().sel, sums_.device(), n);
        timer.mark(1);
        HIP_CHECK(hipStreamSynchronize(s));
        timer.read(&select_sum_ms_);
    } catch (...) {
        (void)hipStreamSynchronize(cur().stream.get());
        bind_selectors(prev, prev_n, prev_form);
        throw;
    }
    bind_selectors(prev, prev_n, prev_form);
    for (size_t i = 0; i < n; ++i) read_slot(slots[i], out + i * p_.lwe_len());
}

}  // namespace fr
