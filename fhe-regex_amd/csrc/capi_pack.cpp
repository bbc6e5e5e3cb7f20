// C-ABI entries of the packed results (include/fheregex.h): the packing keyswitch of boolean
// handles into one GLWE ciphertext under the client's key, its wire blob and its decryption; the
// one pack-to-blob step every reply goes through (pack_rows, pack_to_blob) and the mapped-pack hooks.
#include <cmath>
#include <cstring>
#include <vector>

#include "ctx.h"

using namespace fr;

// every handle is checked before anything runs; a boolean is one slot or a trivial value
static std::vector<DevGate> bool_rows(fr_ctx* ctx, const fr_ct* bools, size_t n, const char* not_bool) {
    std::vector<DevGate> rows(n);
    for (size_t j = 0; j < n; ++j) rows[j] = bool_gate(ctx->get(bools[j]), not_bool);
    return rows;
}
// the rows of fr_pack_bools' n handles, after its refusals
static std::vector<DevGate> handle_rows(fr_ctx* ctx, const fr_ct* bools, size_t n) {
    NEED(ctx && bools);
    NEED(n >= 1 && n <= (size_t)ctx->p.N);
    ctx->need_packing_key();
    return bool_rows(ctx, bools, n, "fr_pack_bools: every handle must be a boolean");
}
// the packing key's rows on the host: a host-only context's own, else a copy for this call
static const uint64_t* host_packing_key(fr_ctx* ctx, std::vector<uint64_t>& copy) {
    if (!ctx->dev) return ctx->pksk.data();
    copy.resize(pk_len(ctx->p));
    ctx->dev->download_packing_key(copy.data());
    return copy.data();
}

void fr::pack_rows(fr_ctx* ctx, const DevGate* rows, size_t n_rows, const int32_t* map, size_t n, uint64_t* words,
                   uint16_t* v) {
    if (ctx->dev && map) return ctx->dev->pack_mapped(rows, n_rows, map, n, words, v);
    if (ctx->dev && v) return ctx->dev->pack_bools_compact(rows, n, v);
    if (ctx->dev) return ctx->dev->pack_bools(rows, n, words);
    std::vector<int32_t> off(n), w(n, 0);  // trivial handles only: no row reads a slot
    for (size_t j = 0; j < n; ++j) off[j] = rows[j].offset;
    std::vector<uint64_t> full(v ? pk_row_words(ctx->p) : 0);
    if (v) words = full.data();
    pack_host(ctx->p, ctx->pksk.data(), nullptr, w.data(), off.data(), n, words);
    for (size_t t = 0; v && t < packed_compact_values(ctx->p, n); ++t) v[t] = packed_round16(words[t]);
}

size_t fr::pack_to_blob(fr_ctx* ctx, const DevGate* rows, size_t n_rows, const int32_t* map, size_t n, bool compact,
                        uint8_t* buf) {
    std::vector<uint16_t> v(compact ? packed_compact_values(ctx->p, n) : 0);
    std::vector<uint64_t> words(compact ? 0 : pk_row_words(ctx->p));
    if (n_rows) pack_rows(ctx, rows, n_rows, map, n, compact ? nullptr : words.data(), compact ? v.data() : nullptr);
    if (compact) write_packed_compact(ctx->p, n, v.data(), buf);
    else write_packed_result(ctx->p, n, words.data(), buf);
    return compact ? packed_compact_size(ctx->p, n) : packed_result_size(ctx->p);
}

// fr_pack_bools_blob and fr_pack_bools_compact
static int pack_bools_to(fr_ctx* ctx, const fr_ct* bools, size_t n, bool compact, uint8_t* buf, size_t cap,
                         size_t* written) {
    FR_TRY({
        NEED(ctx && written);
        NEED(n >= 1 && n <= (size_t)ctx->p.N);
        if (answer_size(written, compact ? packed_compact_size(ctx->p, n) : packed_result_size(ctx->p), buf, cap))
            return FR_OK;
        pack_to_blob(ctx, handle_rows(ctx, bools, n).data(), n, nullptr, n, compact, buf);
    })
}

extern "C" {

int fr_packed_result_size(fr_ctx* ctx, size_t n, size_t* bytes) {
    FR_TRY({
        NEED(ctx && bytes);
        NEED(n >= 1 && n <= (size_t)ctx->p.N);
        *bytes = packed_result_size(ctx->p);
    })
}

int fr_pack_bools(fr_ctx* ctx, const fr_ct* bools, size_t n, uint64_t* out_words) {
    FR_TRY({
        NEED(out_words);
        pack_rows(ctx, handle_rows(ctx, bools, n).data(), n, nullptr, n, out_words, nullptr);
    })
}

int fr_pack_bools_blob(fr_ctx* ctx, const fr_ct* bools, size_t n, uint8_t* buf, size_t cap, size_t* written) {
    return pack_bools_to(ctx, bools, n, false, buf, cap, written);
}

int fr_packed_compact_size(fr_ctx* ctx, size_t n, size_t* bytes) {
    FR_TRY({
        NEED(ctx && bytes);
        NEED(n >= 1 && n <= (size_t)ctx->p.N);
        *bytes = packed_compact_size(ctx->p, n);
    })
}

int fr_pack_bools_compact(fr_ctx* ctx, const fr_ct* bools, size_t n, uint8_t* buf, size_t cap, size_t* written) {
    return pack_bools_to(ctx, bools, n, true, buf, cap, written);
}

int fr_compress_packed(fr_ctx* ctx, const uint64_t* words, size_t n, uint8_t* buf, size_t cap, size_t* written) {
    FR_TRY({
        NEED(ctx && written);
        NEED(n >= 1 && n <= (size_t)ctx->p.N);
        const size_t need = packed_compact_size(ctx->p, n);
        *written = need;
        if (!buf) return FR_OK;  // size query
        NEED(words && cap >= need);
        compress_packed(ctx->p, n, words, buf);
    })
}

int fr_expand_packed_compact(fr_ctx* ctx, const uint8_t* blob, size_t len, uint64_t* words, size_t* n) {
    FR_TRY({
        NEED(ctx && blob && n);
        *n = check_packed_compact(ctx->p, blob, len);  // before anything is written
        if (words) expand_packed_compact(ctx->p, blob, len, words);
    })
}

int fr_decrypt_packed_compact(fr_ctx* ctx, const uint8_t* blob, size_t len, uint8_t* bits, size_t* n) {
    FR_TRY({
        NEED(ctx && blob && n);
        // the blob is checked before anything is allocated
        const size_t nb = check_packed_compact(ctx->p, blob, len);
        *n = nb;
        if (!bits) return FR_OK;  // size query
        if (!ctx->has_ck) throw Error(FR_ERR_NO_KEY, "client key not loaded");
        std::vector<uint64_t> ct(pk_row_words(ctx->p)), phase((size_t)ctx->p.N);
        expand_packed_compact(ctx->p, blob, len, ct.data());
        glwe_phase(ctx->p, ctx->ck, ct.data(), phase.data());
        const uint64_t half = 1ULL << (DELTA_LOG - 1);
        // (the coefficients past n were not sent: nothing to check there)
        for (size_t j = 0; j < nb; ++j) bits[j] = (uint8_t)(((phase[j] + half) >> DELTA_LOG) & 1);
    })
}

int fr_pack_lwes(fr_ctx* ctx, const uint64_t* lwes, const int32_t* w, const int32_t* off, size_t n,
                 uint64_t* out_words) {
    FR_TRY({
        NEED(ctx && out_words && (lwes || w));
        NEED(n >= 1 && n <= (size_t)ctx->p.N);
        if (!lwes)
            for (size_t j = 0; j < n; ++j) NEED(w[j] == 0);
        ctx->need_packing_key();
        std::vector<uint64_t> copy;
        pack_host(ctx->p, host_packing_key(ctx, copy), lwes, w, off, n, out_words);
    })
}

int fr_pack_lwes_mapped(fr_ctx* ctx, const uint64_t* lwes, const int32_t* w, const int32_t* off, size_t n_rows,
                        const int32_t* map, size_t n, uint64_t* out_words) {
    FR_TRY({
        NEED(ctx && out_words && map && (lwes || w));
        if (!lwes)
            for (size_t r = 0; r < n_rows; ++r) NEED(w[r] == 0);
        ctx->need_packing_key();
        check_pack_map(map, n, n_rows, (size_t)ctx->p.N);
        std::vector<uint64_t> copy;
        pack_host_mapped(ctx->p, host_packing_key(ctx, copy), lwes, w, off, n_rows, map, n, out_words);
    })
}

int fr_dev_pack_mapped(fr_ctx* ctx, const fr_ct* bools, size_t n_rows, const int32_t* map, size_t n, int32_t compact,
                       uint8_t* buf, size_t cap, size_t* written) {
    FR_TRY({
        NEED(ctx && bools && map && written && (compact == 0 || compact == 1));
        NEED(n >= 1 && n <= (size_t)ctx->p.N);
        ctx->device();
        if (answer_size(written, compact ? packed_compact_size(ctx->p, n) : packed_result_size(ctx->p), buf, cap))
            return FR_OK;
        check_pack_map(map, n, n_rows, (size_t)ctx->p.N);  // (before bools is read: n_rows of them)
        const std::vector<DevGate> rows =
            bool_rows(ctx, bools, n_rows, "fr_dev_pack_mapped: every handle must be a boolean");
        pack_to_blob(ctx, rows.data(), n_rows, map, n, compact != 0, buf);
    })
}

int fr_packed_phase(fr_ctx* ctx, const uint64_t* words, uint64_t* phase) {
    FR_TRY({
        NEED(ctx && words && phase);
        if (!ctx->has_ck) throw Error(FR_ERR_NO_KEY, "client key not loaded");
        glwe_phase(ctx->p, ctx->ck, words, phase);
    })
}

int fr_decrypt_packed(fr_ctx* ctx, const uint8_t* blob, size_t len, uint8_t* bits, size_t* n) {
    FR_TRY({
        NEED(ctx && blob && n);
        // the blob is checked before anything is allocated
        const size_t nb = check_packed_result(ctx->p, blob, len);
        *n = nb;
        if (!bits) return FR_OK;  // size query
        if (!ctx->has_ck) throw Error(FR_ERR_NO_KEY, "client key not loaded");
        const size_t W = pk_row_words(ctx->p), N = (size_t)ctx->p.N;
        std::vector<uint64_t> ct(W), phase(N);
        std::memcpy(ct.data(), blob + PKRES_HEADER, 8 * W);  // (a little-endian host)
        glwe_phase(ctx->p, ctx->ck, ct.data(), phase.data());
        const uint64_t half = 1ULL << (DELTA_LOG - 1);
        for (size_t j = 0; j < N; ++j) {
            const uint64_t m = (phase[j] + half) >> DELTA_LOG;  // round(phase / Delta) mod 32
            if (j < nb) bits[j] = (uint8_t)(m & 1);
            else if (m != 0) throw Error(FR_ERR_INVALID, "packed result: a coefficient past n does not decrypt to 0");
        }
    })
}

int fr_dev_packing_limb_column(fr_ctx* ctx, int32_t col, uint64_t* out) {
    FR_TRY({
        NEED(ctx && out);
        ctx->need_packing_key();
        ctx->device().packing_limb_column(col, out);
    })
}

int fr_device_timers_pack(fr_ctx* ctx, double* ms) {
    FR_TRY({
        NEED(ctx && ms);
        std::memcpy(ms, ctx->device().pack_ms(), 3 * sizeof(double));
    })
}

int fr_device_timers_pack_compact(fr_ctx* ctx, double* ms) {
    FR_TRY({
        NEED(ctx && ms);
        std::memcpy(ms, ctx->device().pack_ms(), 4 * sizeof(double));
    })
}

}  // extern "C"
