// C-ABI entries of the client side and the keys (include/fheregex.h): client, server and
// packing keys, encryption, the radix wire format, decryption.
#include <cstring>
#include <vector>

#include "ctx.h"

using namespace fr;

extern "C" {

int fr_load_client_key(fr_ctx* ctx, const uint8_t* data, size_t len) {
    FR_TRY({
        NEED(ctx && data);
        ClientKey ck = parse_client_key(data, len);
        if ((size_t)ctx->p.k * ctx->p.N != ck.s_big.size() || (size_t)ctx->p.n != ck.s_small.size())
            throw Error(FR_ERR_INVALID, "client key dimensions do not match the context params");
        // the radix encoding this build implements: PARAM_MESSAGE_2_CARRY_2, 4 blocks per
        // character (ciphertext.rs:1,12-13,43-44); a key of other parameters would decode wrong
        if (ck.message_modulus != MESSAGE_MODULUS || ck.carry_modulus != CARRY_MODULUS || ck.num_blocks != 4)
            throw Error(FR_ERR_INVALID, "client key: message/carry modulus or block count other than "
                                        "PARAM_MESSAGE_2_CARRY_2 with 4 blocks");
        ctx->ck = std::move(ck);
        ctx->has_ck = true;
        ctx->has_sk = false;
    })
}

// Every draw below runs under one RngKey (chacha.h).  A seeded entry point and its keyed twin hand
// their KeySource to one body, which checks its preconditions and then draws the key: from_seed,
// from_bytes, or from_os for a NULL key.  The host copy of the key is wiped on the way out.
namespace {
struct KeySource {
    bool seeded;
    uint64_t seed = 0;
    const uint8_t* key32 = nullptr;
    KeySource(uint64_t s) : seeded(true), seed(s) {}
    KeySource(const uint8_t* k) : seeded(false), key32(k) {}
};
struct ScopedKey {
    RngKey k;
    explicit ScopedKey(const KeySource& s)
        : k(s.seeded ? RngKey::from_seed(s.seed) : s.key32 ? RngKey::from_bytes(s.key32) : RngKey::from_os()) {}
    ~ScopedKey() { wipe_key(k); }
    ScopedKey(const ScopedKey&) = delete;
    ScopedKey& operator=(const ScopedKey&) = delete;
};
}  // namespace

static void gen_client_key_from(fr_ctx* ctx, KeySource src) {
    NEED(ctx);
    ScopedKey key(src);
    ctx->ck = gen_client_key(ctx->p, key.k);
    ctx->has_ck = true;
    ctx->has_sk = false;
}

int fr_gen_client_key(fr_ctx* ctx, uint64_t seed) { FR_TRY(gen_client_key_from(ctx, seed)) }
int fr_gen_client_key_keyed(fr_ctx* ctx, const uint8_t* key32) { FR_TRY(gen_client_key_from(ctx, key32)) }

int fr_serialize_client_key(fr_ctx* ctx, uint8_t* buf, size_t cap, size_t* written) {
    FR_TRY({
        NEED(ctx && written);
        if (!ctx->has_ck) throw Error(FR_ERR_NO_KEY, "client key not loaded");
        const std::vector<uint8_t> b = serialize_client_key(ctx->ck);
        if (answer_size(written, b.size(), buf, cap)) return FR_OK;
        std::memcpy(buf, b.data(), b.size());
    })
}

// where the server key is generated (fr_set_keygen); checked before a key is drawn
static bool server_keygen_on_device(fr_ctx* ctx) {
    if (!ctx->has_ck) throw Error(FR_ERR_NO_KEY, "client key not loaded");
    const bool on_dev = ctx->dev && ctx->p.ring == FR_RING_FFT && ctx->keygen != FR_KEYGEN_HOST;
    if (ctx->keygen == FR_KEYGEN_DEVICE && !on_dev)
        throw Error(ctx->dev ? FR_ERR_INVALID : FR_ERR_NO_DEVICE, "device keygen needs a device and the FFT ring");
    return on_dev;
}
static void gen_server_key_from(fr_ctx* ctx, KeySource src, bool compact) {
    NEED(ctx);
    const bool on_dev = server_keygen_on_device(ctx);
    ScopedKey scoped(src);  // after the preconditions: a NULL key draws from the OS
    const RngKey& key = scoped.k;
    if (compact && ctx->p.ring != FR_RING_FFT) throw Error(FR_ERR_INVALID, "compact server key: FFT ring only");
    ctx->has_sk = false;
    ctx->sk_compact = false;
    if (on_dev) {
        ctx->ksk.clear();
        ctx->bsk.clear();
        if (compact) {
            // only the public mask key goes to the device; the noise is drawn here under `key`
            ctx->mask_key = derive_mask_key(key);
            ctx->dev->gen_server_key(ctx->ck, key, &ctx->mask_key);
        } else {
            ctx->dev->gen_server_key(ctx->ck, key);
        }
    } else {
        if (compact) {
            gen_server_key_compact(ctx->p, ctx->ck, key, ctx->ksk, ctx->bsk, ctx->mask_key);
        } else {
            gen_ksk(ctx->p, ctx->ck, key, ctx->ksk);
            gen_bsk(ctx->p, ctx->ck, key, ctx->bsk);
        }
        if (ctx->dev) ctx->dev->upload_keys(ctx->ksk, ctx->bsk);
    }
    ctx->sk_on_device = on_dev;
    ctx->sk_compact = compact;
    ctx->has_sk = true;
}

int fr_gen_server_key(fr_ctx* ctx, uint64_t seed) { FR_TRY(gen_server_key_from(ctx, seed, false)) }
int fr_gen_server_key_keyed(fr_ctx* ctx, const uint8_t* key32) { FR_TRY(gen_server_key_from(ctx, key32, false)) }
int fr_gen_server_key_compact(fr_ctx* ctx, uint64_t seed) { FR_TRY(gen_server_key_from(ctx, seed, true)) }
int fr_gen_server_key_compact_keyed(fr_ctx* ctx, const uint8_t* key32) { FR_TRY(gen_server_key_from(ctx, key32, true)) }

int fr_server_key_sizes(fr_ctx* ctx, size_t* ksk_len, size_t* bsk_len) {
    FR_TRY({
        NEED(ctx);
        const Params& p = ctx->p;
        if (ksk_len) *ksk_len = p.ksk_len();
        if (bsk_len) *bsk_len = p.bsk_len();
    })
}

int fr_export_server_key(fr_ctx* ctx, uint64_t* ksk, size_t ksk_len, uint64_t* bsk, size_t bsk_len) {
    FR_TRY({
        NEED(ctx);
        if (!ctx->has_sk) throw Error(FR_ERR_NO_KEY, "server key not generated");
        if (ctx->sk_on_device) {
            ctx->device().download_server_key(ksk, ksk_len, bsk, bsk_len);
            return FR_OK;
        }
        if (ksk) {
            NEED(ksk_len == ctx->ksk.size());
            std::memcpy(ksk, ctx->ksk.data(), 8 * ksk_len);
        }
        if (bsk) {
            NEED(bsk_len == ctx->bsk.size());
            std::memcpy(bsk, ctx->bsk.data(), 8 * bsk_len);
        }
    })
}

int fr_load_server_key(fr_ctx* ctx, const uint64_t* ksk, size_t ksk_len, const uint64_t* bsk, size_t bsk_len) {
    FR_TRY({
        NEED(ctx && ksk && bsk);
        const Params& p = ctx->p;
        if (ksk_len != p.ksk_len() || bsk_len != p.bsk_len())
            throw Error(FR_ERR_INVALID, "server key lengths do not match the context params (fr_server_key_sizes)");
        ctx->has_sk = false;
        ctx->sk_compact = false;
        std::vector<uint64_t> k(ksk, ksk + ksk_len), b(bsk, bsk + bsk_len);
        if (ctx->dev) ctx->dev->upload_keys(k, b);
        ctx->ksk = std::move(k);
        ctx->bsk = std::move(b);
        ctx->sk_on_device = false;
        ctx->has_sk = true;
    })
}

int fr_server_key_compact_size(fr_ctx* ctx, size_t* bytes) {
    FR_TRY({
        NEED(ctx && bytes);
        if (ctx->p.ring != FR_RING_FFT) throw Error(FR_ERR_INVALID, "compact server key: FFT ring only");
        *bytes = compact_size(ctx->p);
    })
}

int fr_export_server_key_compact(fr_ctx* ctx, uint8_t* buf, size_t cap, size_t* written) {
    FR_TRY({
        NEED(ctx && written);
        if (!ctx->has_sk) throw Error(FR_ERR_NO_KEY, "server key not generated");
        if (!ctx->sk_compact)
            throw Error(FR_ERR_INVALID, "the installed server key was not generated in compact form: its masks are "
                                        "not expandable from a mask key (fr_gen_server_key_compact)");
        const size_t need = compact_size(ctx->p);
        if (answer_size(written, need, buf, cap)) return FR_OK;
        if (ctx->sk_on_device) {
            std::vector<uint64_t> k(ctx->p.ksk_len()), b(ctx->p.bsk_len());
            ctx->device().download_server_key(k.data(), k.size(), b.data(), b.size());
            pack_compact(ctx->p, ctx->mask_key, k, b, buf);
        } else {
            pack_compact(ctx->p, ctx->mask_key, ctx->ksk, ctx->bsk, buf);
        }
    })
}

int fr_load_server_key_compact(fr_ctx* ctx, const uint8_t* blob, size_t len) {
    FR_TRY({
        NEED(ctx && blob);
        // length, magic and parameters are checked before the installed key is touched
        const RngKey mk = check_compact(ctx->p, blob, len);
        if (ctx->dev) {
            ctx->has_sk = false;
            ctx->dev->load_server_key_compact(mk, blob + COMPACT_HEADER);
            ctx->ksk.clear();
            ctx->bsk.clear();
            ctx->sk_on_device = true;
        } else {
            std::vector<uint64_t> k, b;
            expand_compact(ctx->p, blob, len, k, b);
            ctx->has_sk = false;
            ctx->ksk = std::move(k);
            ctx->bsk = std::move(b);
            ctx->sk_on_device = false;
        }
        ctx->mask_key = mk;
        ctx->sk_compact = true;
        ctx->has_sk = true;
    })
}

// ---- packing key (keys.h): optional, beside the server key; nothing else depends on it

// checked before a key is drawn
static void check_gen_packing_key(fr_ctx* ctx) {
    NEED(ctx);
    if (!ctx->has_ck) throw Error(FR_ERR_NO_KEY, "client key not loaded");
    if (ctx->keygen == FR_KEYGEN_DEVICE && !ctx->dev) throw Error(FR_ERR_NO_DEVICE, "device keygen needs a device");
}

// compact: the compact form (keys.h) -- the masks under the public mask key, which is all a
// kernel sees; the noise under `key` on the host either way
static void gen_packing_key_from(fr_ctx* ctx, KeySource src, bool compact) {
    check_gen_packing_key(ctx);
    ScopedKey scoped(src);
    const RngKey& key = scoped.k;
    const bool on_dev = ctx->dev && ctx->keygen != FR_KEYGEN_HOST;
    RngKey mk{};  // public; the secret key is never copied
    if (compact) mk = derive_mask_key(key);
    const RngKey& mask = compact ? mk : key;
    ctx->has_pk = false;
    ctx->pk_compact = false;
    if (on_dev) {
        ctx->pksk.clear();
        ctx->pksk.shrink_to_fit();
        ctx->dev->gen_packing_key(ctx->ck, mask, key, compact);
    } else {
        // the whole key through the row generator: kN^2 / 2 additions per row on every host
        // thread, a few seconds in all
        ctx->pksk.resize(pk_len(ctx->p));
        gen_packing_rows(ctx->p, ctx->ck, mask, key, compact, 0, pk_rows(ctx->p), ctx->pksk.data());
        if (ctx->dev) {
            ctx->dev->upload_packing_key(ctx->pksk.data());
            ctx->pksk.clear();
            ctx->pksk.shrink_to_fit();
        }
    }
    if (compact) ctx->pk_mask_key = mask;
    ctx->pk_compact = compact;
    ctx->has_pk = true;
}

int fr_gen_packing_key(fr_ctx* ctx, uint64_t seed) { FR_TRY(gen_packing_key_from(ctx, seed, false)) }
int fr_gen_packing_key_keyed(fr_ctx* ctx, const uint8_t* key32) { FR_TRY(gen_packing_key_from(ctx, key32, false)) }
int fr_gen_packing_key_compact(fr_ctx* ctx, uint64_t seed) { FR_TRY(gen_packing_key_from(ctx, seed, true)) }
int fr_gen_packing_key_compact_keyed(fr_ctx* ctx, const uint8_t* key32) { FR_TRY(gen_packing_key_from(ctx, key32, true)) }

static void gen_packing_rows_with(fr_ctx* ctx, const uint8_t* key32, bool compact, size_t row_lo, size_t row_hi,
                                  uint64_t* out) {
    NEED(ctx && row_lo <= row_hi && row_hi <= pk_rows(ctx->p) && (out || row_lo == row_hi));
    if (!ctx->has_ck) throw Error(FR_ERR_NO_KEY, "client key not loaded");
    ScopedKey key(key32);
    RngKey mk{};
    if (compact) mk = derive_mask_key(key.k);
    const RngKey& mask = compact ? mk : key.k;
    gen_packing_rows(ctx->p, ctx->ck, mask, key.k, compact, row_lo, row_hi, out);
}

int fr_gen_packing_rows_keyed(fr_ctx* ctx, const uint8_t* key32, size_t row_lo, size_t row_hi, uint64_t* out) {
    FR_TRY(gen_packing_rows_with(ctx, key32, false, row_lo, row_hi, out))
}

int fr_gen_packing_rows_compact_keyed(fr_ctx* ctx, const uint8_t* key32, size_t row_lo, size_t row_hi, uint64_t* out) {
    FR_TRY(gen_packing_rows_with(ctx, key32, true, row_lo, row_hi, out))
}

int fr_packing_key_size(fr_ctx* ctx, size_t* bytes) {
    FR_TRY({
        NEED(ctx && bytes);
        *bytes = pk_blob_size(ctx->p);
    })
}

int fr_export_packing_key(fr_ctx* ctx, uint8_t* buf, size_t cap, size_t* written) {
    FR_TRY({
        NEED(ctx && written);
        if (!ctx->has_pk) throw Error(FR_ERR_INVALID, "no packing key (fr_gen_packing_key, fr_load_packing_key)");
        const size_t need = pk_blob_size(ctx->p);
        if (answer_size(written, need, buf, cap)) return FR_OK;
        write_pk_header(ctx->p, buf);
        // (a little-endian host: the rows are their wire form; PK_HEADER is a multiple of 8, but
        // buf may sit anywhere)
        if (ctx->dev) {
            std::vector<uint64_t> rows(pk_len(ctx->p));
            ctx->dev->download_packing_key(rows.data());
            std::memcpy(buf + PK_HEADER, rows.data(), 8 * rows.size());
        } else {
            std::memcpy(buf + PK_HEADER, ctx->pksk.data(), 8 * ctx->pksk.size());
        }
    })
}

int fr_load_packing_key(fr_ctx* ctx, const uint8_t* blob, size_t len) {
    FR_TRY({
        NEED(ctx && blob);
        // length, magic, parameters and gadget are checked before the installed key is touched
        check_pk_blob(ctx->p, blob, len);
        if (ctx->dev) {
            ctx->has_pk = false;
            ctx->pk_compact = false;
            ctx->dev->upload_packing_key(blob + PK_HEADER);  // drains every lane first
        } else {
            std::vector<uint64_t> rows(pk_len(ctx->p));
            std::memcpy(rows.data(), blob + PK_HEADER, 8 * rows.size());
            ctx->pksk = std::move(rows);
        }
        ctx->pk_compact = false;
        ctx->has_pk = true;
    })
}

// ---- compact packing key (keys.h): the mask key and the 40-bit bodies travel

int fr_packing_key_compact_size(fr_ctx* ctx, size_t* bytes) {
    FR_TRY({
        NEED(ctx && bytes);
        *bytes = pk_compact_size(ctx->p);
    })
}

int fr_export_packing_key_compact(fr_ctx* ctx, uint8_t* buf, size_t cap, size_t* written) {
    FR_TRY({
        NEED(ctx && written);
        if (!ctx->has_pk) throw Error(FR_ERR_INVALID, "no packing key (fr_gen_packing_key, fr_load_packing_key)");
        if (!ctx->pk_compact)
            throw Error(FR_ERR_INVALID, "the installed packing key was not generated in compact form: its masks are "
                                        "not expandable from a mask key (fr_gen_packing_key_compact)");
        const size_t need = pk_compact_size(ctx->p);
        if (answer_size(written, need, buf, cap)) return FR_OK;
        write_pk_compact_header(ctx->p, ctx->pk_mask_key, buf);
        // the device gathers the planes from its resident rows: 5 of every 8 (k+1) bytes come back
        if (ctx->dev) ctx->dev->download_packing_key_compact(buf + PKC_HEADER);
        else pack_pk_compact(ctx->p, ctx->pksk.data(), buf + PKC_HEADER);
    })
}

int fr_load_packing_key_compact(fr_ctx* ctx, const uint8_t* blob, size_t len) {
    FR_TRY({
        NEED(ctx && blob);
        // the whole header is checked before the installed key is touched or anything is allocated
        const RngKey mk = check_pk_compact(ctx->p, blob, len);
        if (ctx->dev) {
            ctx->has_pk = false;
            ctx->pk_compact = false;
            ctx->dev->load_packing_key_compact(mk, blob + PKC_HEADER);  // drains every lane first
        } else {
            std::vector<uint64_t> rows;
            expand_pk_compact(ctx->p, blob, len, rows);
            ctx->pksk = std::move(rows);
        }
        ctx->pk_mask_key = mk;
        ctx->pk_compact = true;
        ctx->has_pk = true;
    })
}

// (the preconditions are checked before a key is drawn)
static void encrypt_blocks_from(fr_ctx* ctx, const uint8_t* msgs, size_t count, KeySource src, uint64_t first_block,
                                uint64_t* out) {
    NEED(ctx && (msgs || !count) && (out || !count));
    if (!ctx->has_ck) throw Error(FR_ERR_NO_KEY, "client key not loaded");
    for (size_t i = 0; i < count; ++i) NEED(msgs[i] < 16);
    ScopedKey key(src);
    encrypt_blocks(ctx->p, ctx->ck, msgs, count, key.k, first_block, out);
}

int fr_encrypt_blocks(fr_ctx* ctx, const uint8_t* msgs, size_t count, uint64_t seed, uint64_t first_block,
                      uint64_t* out) {
    FR_TRY(encrypt_blocks_from(ctx, msgs, count, seed, first_block, out))
}
int fr_encrypt_blocks_keyed(fr_ctx* ctx, const uint8_t* msgs, size_t count, const uint8_t* key32,
                            uint64_t first_block, uint64_t* out) {
    FR_TRY(encrypt_blocks_from(ctx, msgs, count, key32, first_block, out))
}

// radix messages of a string (ciphertext.rs:18-29: 4 blocks of 2 bits, least significant first)

static std::vector<uint8_t> str_blocks(const char* s, size_t len) {
    std::vector<uint8_t> msgs(4 * len);
    for (size_t i = 0; i < len; ++i) {
        const uint8_t c = (uint8_t)s[i];
        if (c > 127) throw Error(FR_ERR_NON_ASCII, "content contains non-ascii characters");
        for (int b = 0; b < 4; ++b) msgs[4 * i + b] = (c >> (2 * b)) & 3;
    }
    return msgs;
}

static void encrypt_str_from(fr_ctx* ctx, const char* s, size_t len, KeySource src, uint64_t* out) {
    NEED(ctx && (s || !len) && (out || !len));
    if (!ctx->has_ck) throw Error(FR_ERR_NO_KEY, "client key not loaded");
    const std::vector<uint8_t> msgs = str_blocks(s, len);
    ScopedKey key(src);
    encrypt_blocks(ctx->p, ctx->ck, msgs.data(), msgs.size(), key.k, 0, out);
}

int fr_encrypt_str(fr_ctx* ctx, const char* s, size_t len, uint64_t seed, uint64_t* out) {
    FR_TRY(encrypt_str_from(ctx, s, len, seed, out))
}
int fr_encrypt_str_keyed(fr_ctx* ctx, const char* s, size_t len, const uint8_t* key32, uint64_t* out) {
    FR_TRY(encrypt_str_from(ctx, s, len, key32, out))
}

// preconditions before the key is drawn, in this order: client key, device, ASCII content
static void encrypt_upload_from(fr_ctx* ctx, const char* s, size_t len, KeySource src, fr_ct* out) {
    NEED(ctx && (s || !len) && (out || !len));
    if (!ctx->has_ck) throw Error(FR_ERR_NO_KEY, "client key not loaded");
    Device& dev = ctx->device();
    const std::vector<uint8_t> msgs = str_blocks(s, len);
    ScopedKey key(src);
    Slots slots(dev, msgs.size());
    dev.encrypt_to_slots(ctx->ck, msgs.data(), msgs.size(), key.k, 0, slots.data());
    ctx->adopt(std::move(slots), true, out);
}

int fr_encrypt_upload_str(fr_ctx* ctx, const char* s, size_t len, uint64_t seed, fr_ct* out) {
    FR_TRY(encrypt_upload_from(ctx, s, len, seed, out))
}
int fr_encrypt_upload_str_keyed(fr_ctx* ctx, const char* s, size_t len, const uint8_t* key32, fr_ct* out) {
    FR_TRY(encrypt_upload_from(ctx, s, len, key32, out))
}

// ---- compact (seeded) content (keys.h): the client packs bodies + mask key, the server
// expands them on the host or straight into arena slots

int fr_compact_content_size(fr_ctx* ctx, size_t n_blocks, size_t* bytes) {
    FR_TRY({
        NEED(ctx && bytes);
        *bytes = content_blob_size(n_blocks);
    })
}

// the blob of `msgs` under `key32` (NULL: OS CSPRNG), after the caller's preconditions;
// the size is answered before a key is drawn
static void encrypt_compact_with(fr_ctx* ctx, const std::vector<uint8_t>& msgs, const uint8_t* key32,
                                 uint64_t first_block, uint8_t* buf, size_t cap, size_t* written) {
    check_content_range(first_block, msgs.size());
    const size_t need = content_blob_size(msgs.size());
    if (answer_size(written, need, buf, cap)) return;
    ScopedKey key(key32);
    const std::vector<uint8_t> blob = encrypt_content_blob(ctx->p, ctx->ck, msgs.data(), msgs.size(), key.k, first_block);
    std::memcpy(buf, blob.data(), need);
}

int fr_encrypt_str_compact_keyed(fr_ctx* ctx, const char* s, size_t len, const uint8_t* key32, uint8_t* buf,
                                 size_t cap, size_t* written) {
    FR_TRY({
        NEED(ctx && (s || !len) && written);
        if (!ctx->has_ck) throw Error(FR_ERR_NO_KEY, "client key not loaded");
        const std::vector<uint8_t> msgs = str_blocks(s, len);
        encrypt_compact_with(ctx, msgs, key32, 0, buf, cap, written);
    })
}

int fr_encrypt_blocks_compact_keyed(fr_ctx* ctx, const uint8_t* msgs, size_t count, const uint8_t* key32,
                                    uint64_t first_block, uint8_t* buf, size_t cap, size_t* written) {
    FR_TRY({
        NEED(ctx && (msgs || !count) && written);
        if (!ctx->has_ck) throw Error(FR_ERR_NO_KEY, "client key not loaded");
        for (size_t i = 0; i < count; ++i) NEED(msgs[i] < 16);
        const std::vector<uint8_t> m(msgs, msgs + count);
        encrypt_compact_with(ctx, m, key32, first_block, buf, cap, written);
    })
}

int fr_expand_compact_content(fr_ctx* ctx, const uint8_t* blob, size_t len, uint64_t* out, size_t out_words,
                              size_t* n_blocks) {
    FR_TRY({
        NEED(ctx && blob && n_blocks);
        const ContentBlob c = check_content_blob(ctx->p, blob, len, false);
        *n_blocks = c.n_blocks;
        if (!out) return FR_OK;  // size query
        // (n_blocks <= (len - 64) / 8: the product cannot wrap)
        NEED(out_words >= c.n_blocks * (size_t)ctx->p.lwe_len());
        expand_content(ctx->p, blob, len, out);
    })
}

// the blob and cap are checked before the device is asked for and before anything is allocated
static void upload_compact(fr_ctx* ctx, const uint8_t* blob, size_t len, bool radix, fr_ct* out, size_t cap,
                           size_t* n) {
    NEED(ctx && blob && n);
    const ContentBlob c = check_content_blob(ctx->p, blob, len, radix);
    const size_t handles = radix ? c.n_blocks / 4 : c.n_blocks;
    *n = handles;
    NEED((out || !handles) && cap >= handles);
    Device& dev = ctx->device();
    ctx->adopt(dev.expand_to_slots(c.mask_key, c.first_block, c.bodies, c.n_blocks), radix, out);
}

int fr_upload_compact_str(fr_ctx* ctx, const uint8_t* blob, size_t len, fr_ct* out, size_t cap, size_t* n_chars) {
    FR_TRY(upload_compact(ctx, blob, len, true, out, cap, n_chars))
}

int fr_upload_compact_blocks(fr_ctx* ctx, const uint8_t* blob, size_t len, fr_ct* out, size_t cap, size_t* n) {
    FR_TRY(upload_compact(ctx, blob, len, false, out, cap, n))
}

// ---- private search (keys.h): the client encrypts the needle's 2 m nibble tables as GLWE
// selectors (bodies + mask key), the server expands them on the host and uploads them once

int fr_needle_size(fr_ctx* ctx, size_t m, size_t* bytes) {
    FR_TRY({
        NEED(ctx && bytes);
        *bytes = needle_blob_size(ctx->p, m);
    })
}

int fr_encrypt_needle_keyed(fr_ctx* ctx, const uint16_t* masks, size_t m, const uint8_t* key32, uint8_t* buf,
                            size_t cap, size_t* written) {
    FR_TRY({
        NEED(ctx && masks && written);
        if (ctx->p.ring != FR_RING_FFT) throw Error(FR_ERR_INVALID, "private search: FFT ring only");
        if (!ctx->has_ck) throw Error(FR_ERR_NO_KEY, "client key not loaded");
        const size_t need = needle_blob_size(ctx->p, m);
        if (answer_size(written, need, buf, cap)) return FR_OK;
        ScopedKey key(key32);
        const std::vector<uint8_t> blob = encrypt_needle_blob(ctx->p, ctx->ck, masks, m, key.k);
        std::memcpy(buf, blob.data(), need);
    })
}

int fr_expand_needle(fr_ctx* ctx, const uint8_t* blob, size_t len, uint64_t* words, size_t cap_words, size_t* m) {
    FR_TRY({
        NEED(ctx && blob && m);
        const NeedleBlob nb = check_needle_blob(ctx->p, blob, len);
        *m = nb.m;
        if (!words) return FR_OK;  // size query
        NEED(cap_words >= needle_words(ctx->p, nb.m));
        expand_needle(ctx->p, blob, len, words);
    })
}

// ---- byte-table needles (keys.h): one 256-entry table per character, N/256 to a selector

int fr_needle_bytes_size(fr_ctx* ctx, size_t m, size_t* bytes) {
    FR_TRY({
        NEED(ctx && bytes);
        *bytes = needle_bytes_blob_size(ctx->p, m);
    })
}

int fr_encrypt_needle_bytes_keyed(fr_ctx* ctx, const uint8_t* tables, size_t m, const uint8_t* key32, uint8_t* buf,
                                  size_t cap, size_t* written) {
    FR_TRY({
        NEED(ctx && tables && written);
        if (ctx->p.ring != FR_RING_FFT) throw Error(FR_ERR_INVALID, "private search: FFT ring only");
        if (!ctx->has_ck) throw Error(FR_ERR_NO_KEY, "client key not loaded");
        const size_t need = needle_bytes_blob_size(ctx->p, m);
        if (answer_size(written, need, buf, cap)) return FR_OK;
        ScopedKey key(key32);
        const std::vector<uint8_t> blob = encrypt_needle_bytes_blob(ctx->p, ctx->ck, tables, m, key.k);
        std::memcpy(buf, blob.data(), need);
    })
}

int fr_expand_needle_bytes(fr_ctx* ctx, const uint8_t* blob, size_t len, uint64_t* words, size_t cap_words,
                           size_t* m) {
    FR_TRY({
        NEED(ctx && blob && m);
        const NeedleBlob nb = check_needle_bytes_blob(ctx->p, blob, len);
        *m = nb.m;
        if (!words) return FR_OK;  // size query
        NEED(cap_words >= needle_bytes_words(ctx->p, nb.m));
        expand_needle_bytes(ctx->p, blob, len, words);
    })
}

int fr_needle_form(const fr_needle* needle, int32_t* form) {
    FR_TRY({
        NEED(needle && form);
        *form = (int32_t)needle->dev.form;
    })
}

int fr_upload_needle(fr_ctx* ctx, const uint8_t* blob, size_t len, fr_needle** out) {
    FR_TRY({
        NEED(ctx && blob && out);
        if (is_needle_bytes_blob(blob, len)) {  // the other form, told apart by its magic
            const NeedleBlob nb = check_needle_bytes_blob(ctx->p, blob, len);
            Device& dev = ctx->device();
            std::vector<uint64_t> words(needle_bytes_words(ctx->p, nb.m));
            expand_needle_bytes(ctx->p, blob, len, words.data());
            auto nd = std::unique_ptr<fr_needle>(
                new fr_needle{dev.upload_needle(words.data(), nb.m, NEEDLE_BYTES), ctx->p.k, ctx->p.N});
            *out = nd.release();
            return FR_OK;
        }
        // the blob is checked before the device is asked for and before anything is allocated
        const NeedleBlob nb = check_needle_blob(ctx->p, blob, len);
        Device& dev = ctx->device();
        std::vector<uint64_t> words(needle_words(ctx->p, nb.m));  // at most 4 MB
        expand_needle(ctx->p, blob, len, words.data());
        auto nd = std::unique_ptr<fr_needle>(new fr_needle{dev.upload_needle(words.data(), nb.m), ctx->p.k, ctx->p.N});
        *out = nd.release();
    })
}

int fr_needle_len(const fr_needle* needle, size_t* m) {
    FR_TRY({
        NEED(needle && m);
        *m = needle->dev.m;
    })
}

int fr_needle_free(fr_ctx* ctx, fr_needle* needle) {
    FR_TRY({
        NEED(ctx);
        if (needle && needle->dev.dev != ctx->dev.get())
            throw Error(FR_ERR_INVALID, "needle: uploaded to another context");
        delete needle;  // waits for every lane first (DevNeedle)
    })
}

// bincode (fixint, little endian) of tfhe-rs 0.2 RadixCiphertext:
//   u64 n_blocks, then per block: u64 len, len x u64 LWE words, u64 degree,
//   u64 message_modulus, u64 carry_modulus
int fr_radix_serialize(fr_ctx* ctx, const uint64_t* blocks, size_t n_blocks, uint64_t degree, uint8_t* buf,
                       size_t cap, size_t* written) {
    FR_TRY({
        NEED(ctx && (blocks || !n_blocks) && written);
        const size_t L = (size_t)ctx->p.lwe_len();
        const size_t need = 8 + n_blocks * (8 * (L + 4));
        if (answer_size(written, need, buf, cap)) return FR_OK;
        uint8_t* o = buf;
        auto put = [&](uint64_t v) {
            std::memcpy(o, &v, 8);
            o += 8;
        };
        put(n_blocks);
        for (size_t b = 0; b < n_blocks; ++b) {
            put(L);
            std::memcpy(o, blocks + b * L, 8 * L);
            o += 8 * L;
            put(degree);
            put(MESSAGE_MODULUS);
            put(CARRY_MODULUS);
        }
    })
}

int fr_radix_deserialize(fr_ctx* ctx, const uint8_t* buf, size_t len, uint64_t* blocks, size_t max_blocks,
                         size_t* n_blocks) {
    FR_TRY({
        NEED(ctx && buf && n_blocks);
        const size_t L = (size_t)ctx->p.lwe_len();
        size_t off = 0;
        auto get = [&]() -> uint64_t {
            if (off + 8 > len) throw Error(FR_ERR_INVALID, "radix ciphertext: truncated");
            uint64_t v;
            std::memcpy(&v, buf + off, 8);
            off += 8;
            return v;
        };
        const uint64_t nb = get();
        if (nb > (len - 8) / (8 * (L + 4))) throw Error(FR_ERR_INVALID, "radix ciphertext: bad block count");
        *n_blocks = (size_t)nb;
        if (!blocks) return FR_OK;  // size query
        NEED(max_blocks >= nb);
        for (uint64_t b = 0; b < nb; ++b) {
            if (get() != L) throw Error(FR_ERR_INVALID, "radix ciphertext: LWE size does not match the parameters");
            if (off + 8 * L > len) throw Error(FR_ERR_INVALID, "radix ciphertext: truncated");
            std::memcpy(blocks + b * L, buf + off, 8 * L);
            off += 8 * L;
            // the comparison LUTs read clean 2-bit blocks (x0 + 4 x1 in [0, 16)); a block
            // carrying a carry (degree > message_modulus - 1) would decode silently wrong
            if (get() > MESSAGE_MODULUS - 1)
                throw Error(FR_ERR_INVALID, "radix ciphertext: block degree exceeds message_modulus - 1 (carries not propagated)");
            if (get() != MESSAGE_MODULUS || get() != CARRY_MODULUS)
                throw Error(FR_ERR_INVALID, "radix ciphertext: message/carry modulus does not match the parameters");
        }
        if (off != len) throw Error(FR_ERR_INVALID, "radix ciphertext: trailing bytes");
    })
}

int fr_decode_block(fr_ctx* ctx, const uint64_t* lwe, uint32_t* v) {
    FR_TRY({
        NEED(ctx && lwe && v);
        if (!ctx->has_ck) throw Error(FR_ERR_NO_KEY, "client key not loaded");
        *v = decode16(lwe_phase(ctx->p, ctx->ck, lwe));
    })
}

int fr_decrypt_radix(fr_ctx* ctx, const uint64_t* blocks, uint64_t* value) {
    FR_TRY({
        NEED(ctx && blocks && value);
        if (!ctx->has_ck) throw Error(FR_ERR_NO_KEY, "client key not loaded");
        uint64_t v = 0;
        for (int b = 0; b < 4; ++b) {
            uint32_t d = decode16(lwe_phase(ctx->p, ctx->ck, blocks + (size_t)b * ctx->p.lwe_len()));
            v += (uint64_t)(d % 4) << (2 * b);
        }
        *value = v & 0xFF;
    })
}

}  // extern "C"
