// C-ABI entries of the packed results (include/fheregex.h): the packing keyswitch of boolean
// handles into one GLWE ciphertext under the client's key, its wire blob and its decryption.
#include <cmath>
#include <cstring>
#include <vector>

#include "ctx.h"

using namespace fr;

static void need_packing_key(fr_ctx* ctx) {
    if (!ctx->has_pk)
        throw Error(FR_ERR_INVALID, "packing needs a packing key (fr_gen_packing_key, fr_load_packing_key)");
}

// the (k+1) N words of the handles' packed GLWE, or (compact) its blob's k N + n rounded values
static void pack_handles(fr_ctx* ctx, const fr_ct* bools, size_t n, uint64_t* out, uint16_t* compact = nullptr) {
    NEED(ctx && bools && (out || compact));
    NEED(n >= 1 && n <= (size_t)ctx->p.N);
    need_packing_key(ctx);
    // every handle is checked before anything runs; a boolean is one slot or a trivial value
    std::vector<DevGate> gates(n);
    std::vector<int32_t> off(n), w(n, 0);
    for (size_t j = 0; j < n; ++j) {
        const HandleRec& h = ctx->get(bools[j]);
        if (!h.is_bool) throw Error(FR_ERR_INVALID, "fr_pack_bools: every handle must be a boolean");
        DevGate& g = gates[j];
        std::memset(&g, 0, sizeof g);
        if (h.b[0].slot >= 0) {
            g.n_in = 1;
            g.in_slot[0] = h.b[0].slot;
            g.in_w[0] = 1;
        } else {
            g.offset = 2 * (h.b[0].triv & 1);  // units of Delta / 2
        }
        off[j] = g.offset;
    }
    if (ctx->dev && compact) return ctx->dev->pack_bools_compact(gates.data(), n, compact);
    if (ctx->dev) return ctx->dev->pack_bools(gates.data(), n, out);
    std::vector<uint64_t> words(compact ? pk_row_words(ctx->p) : 0);
    if (compact) out = words.data();
    pack_host(ctx->p, ctx->pksk.data(), nullptr, w.data(), off.data(), n, out);  // trivial handles only
    for (size_t t = 0; compact && t < packed_compact_values(ctx->p, n); ++t) compact[t] = packed_round16(out[t]);
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
    FR_TRY(pack_handles(ctx, bools, n, out_words))
}

int fr_pack_bools_blob(fr_ctx* ctx, const fr_ct* bools, size_t n, uint8_t* buf, size_t cap, size_t* written) {
    FR_TRY({
        NEED(ctx && written);
        NEED(n >= 1 && n <= (size_t)ctx->p.N);
        const size_t need = packed_result_size(ctx->p);
        *written = need;
        if (!buf) return FR_OK;  // size query
        NEED(cap >= need);
        std::vector<uint64_t> words(pk_row_words(ctx->p));
        pack_handles(ctx, bools, n, words.data());
        write_packed_result(ctx->p, n, words.data(), buf);
    })
}

int fr_packed_compact_size(fr_ctx* ctx, size_t n, size_t* bytes) {
    FR_TRY({
        NEED(ctx && bytes);
        NEED(n >= 1 && n <= (size_t)ctx->p.N);
        *bytes = packed_compact_size(ctx->p, n);
    })
}

int fr_pack_bools_compact(fr_ctx* ctx, const fr_ct* bools, size_t n, uint8_t* buf, size_t cap, size_t* written) {
    FR_TRY({
        NEED(ctx && written);
        NEED(n >= 1 && n <= (size_t)ctx->p.N);
        const size_t need = packed_compact_size(ctx->p, n);
        *written = need;
        if (!buf) return FR_OK;  // size query
        NEED(cap >= need);
        std::vector<uint16_t> v(packed_compact_values(ctx->p, n));
        pack_handles(ctx, bools, n, nullptr, v.data());
        write_packed_compact(ctx->p, n, v.data(), buf);
    })
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
        need_packing_key(ctx);
        if (ctx->dev) {  // the rows live on the device: a host copy for this call
            std::vector<uint64_t> rows(pk_len(ctx->p));
            ctx->dev->download_packing_key(rows.data());
            pack_host(ctx->p, rows.data(), lwes, w, off, n, out_words);
        } else {
            pack_host(ctx->p, ctx->pksk.data(), lwes, w, off, n, out_words);
        }
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
        need_packing_key(ctx);
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
