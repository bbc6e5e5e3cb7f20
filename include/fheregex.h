/*
 * fheregex.h — C-ABI of the MI355X-native gate-bootstrap executor under the
 * homomorphic regex engine of RKlompUU/fhe-regex.
 *
 * The boundary sits exactly where the reference's Execution layer calls into
 * tfhe-rs (the `tfhe::integer::ServerKey` it owns):
 *
 *   reference call site (src/regex/...)              replaced by
 *   ------------------------------------------------ ---------------------------
 *   execution.rs:76   sk.smart_eq(ct_char, ct_const)  fr_eq_const
 *   execution.rs:93   sk.smart_gt(ct_char, ct_const)  fr_gt_const   (ct_ge quirk)
 *   execution.rs:110  sk.smart_le(ct_char, ct_const)  fr_le_const
 *   execution.rs:143  sk.smart_bitand(a, b)           fr_and
 *   execution.rs:173  sk.smart_bitor(a, b)            fr_or
 *   execution.rs:190  sk.smart_bitxor(a, trivial 1)   fr_not
 *   ciphertext.rs:8-30 create_trivial_radix(sk, m)    fr_trivial
 *   ciphertext.rs:42-45 gen_keys_radix(PARAM_MESSAGE_2_CARRY_2, 4)
 *                                                     fr_gen_client_key + fr_gen_server_key
 *   engine.rs:248-254 read_test_keys: bincode::deserialize + ServerKey::new
 *                                                     fr_load_client_key + fr_gen_server_key
 *   engine.rs:238-246 generate_test_keys: bincode::serialize(client key)
 *                                                     fr_serialize_client_key
 *   engine.rs:8 has_match(sk, ...): a server holding only sk
 *                                                     fr_export_server_key -> fr_load_server_key
 *   ciphertext.rs:32-40 encrypt_str / RadixClientKey::encrypt
 *                                                     fr_encrypt_str (client side, test/bench)
 *   mod.rs:17 / engine.rs:289 RadixClientKey::decrypt fr_decrypt_radix (client side)
 *   engine.rs:8-42    has_match(sk, content, pattern) fr_has_match (whole engine, batched)
 *
 * Conventions: every function returns FR_OK (0) or a negative FR_ERR_* code;
 * the message of the last error on this thread is fr_last_error().  No C++
 * exception crosses the ABI.  Ciphertexts are opaque handles (fr_ct) into a
 * device arena owned by the context; inputs are never mutated and every op
 * writes a fresh handle (the reference always passes clones,
 * execution.rs:74-76).  One fr_ctx per GPU, driven by one host thread.
 * Host buffers are caller-owned and copied in or out.
 *
 * LWE layout on the wire: (k*N + 1) little-endian u64 per block, mask then
 * body, torus 2^64, under the reference's flattened GLWE ("big") key; a radix
 * ciphertext is 4 such blocks, least significant 2-bit digit first
 * (ciphertext.rs:18-29).
 */
#ifndef FHEREGEX_H
#define FHEREGEX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    FR_OK = 0,
    FR_ERR_INVALID = -1,      /* bad argument / handle */
    FR_ERR_PARSE = -2,        /* pattern does not parse: reference returns Err (engine.rs:13) */
    FR_ERR_REF_PANIC = -3,    /* the reference would panic (parser.rs:349-351, engine.rs:189-190) */
    FR_ERR_NO_DEVICE = -4,    /* GPU op on a host-only context, or the HIP device is unusable */
    FR_ERR_HIP = -5,          /* HIP runtime error */
    FR_ERR_NO_KEY = -6,       /* client or server key missing */
    FR_ERR_OOM = -7,          /* arena / allocation exhausted */
    FR_ERR_NON_ASCII = -8,    /* encrypt_str on non-ASCII content (ciphertext.rs:33-35) */
    FR_ERR_RNG = -9,          /* the OS CSPRNG gave no randomness (a *_keyed call with a NULL key) */
};

/* Ring of the blind rotation.  FR_RING_FFT: GLWE/GGSW on the
 * 2^64 torus with an f64 negacyclic FFT (tfhe-rs's own representation);
 * FR_RING_RNS: Z_Q[X]/(X^N+1), Q = 998244353 * 1004535809, exact NTTs.  The
 * server key (fr_export_server_key) is a torus BSK for FFT, mod Q for RNS. */
enum { FR_RING_RNS = 0, FR_RING_FFT = 1 };

typedef struct fr_ctx fr_ctx;
typedef uint32_t fr_ct; /* ciphertext handle: a radix (4 blocks), boolean (block 0 + zeros) or trivial */

typedef struct {
    int32_t k;            /* GLWE dimension (reference: 1)            */
    int32_t N;            /* polynomial size (reference: 2048)        */
    int32_t n;            /* small LWE dimension (742)                */
    int32_t ks_base_log;  /* 3 */
    int32_t ks_level;     /* 5 */
    int32_t pbs_base_log; /* 23 */
    int32_t pbs_level;    /* 1 */
    int32_t ring;         /* blind-rotation ring: FR_RING_RNS (0) or FR_RING_FFT (1) */
    double lwe_sigma;
    double glwe_sigma;
} fr_params;

typedef struct {
    uint64_t ct_ops;        /* reference Execution::ct_operations_count (execution.rs:56-58) */
    uint64_t cache_hits;    /* reference Execution::cache_hits (execution.rs:60-62) */
    uint64_t n_branches;    /* variants enumerated by build_branches (engine.rs:15-18) */
    uint64_t pbs;           /* LUT evaluations (gate outputs) executed */
    uint64_t blind_rotations; /* blind rotations (several LUTs may share one: multi-value bootstrapping) */
    uint64_t levels;        /* dependent PBS levels (launch batches) */
    uint64_t max_level_width;
    double host_ms;         /* parse + enumerate + record + lower + compile (plan-cache hit: the lookup) */
    double device_ms;       /* device execution, wall (fr_set_async on: until the launches are enqueued) */
    /* This match's kernel timers (fr_set_profiling on).  Filled only by a blocking call
     * (fr_set_async(ctx, 0)); an asynchronous call returns before its kernels run and
     * leaves them 0: read fr_device_timers after a synchronising call instead. */
    double br_kernel_ms;    /* sum of blind-rotation kernel durations (HIP events) */
    double ks_kernel_ms;    /* sum of lincomb+keyswitch kernel durations (HIP events) */
    uint64_t br_launches;
    uint64_t br_gates;      /* bootstraps across all blind-rotation launches */
    uint64_t plan_cached;   /* 1: the match replayed a cached plan (fr_set_plan_cache) */
} fr_match_stats;

/* ----- context ----- */
/* device >= 0: HIP device ordinal; device == -1: host-only context (parse,
 * record, plan, keygen, plaintext evaluation; GPU ops return FR_ERR_NO_DEVICE). */
int fr_ctx_create(const fr_params* params, int device, fr_ctx** out);
int fr_ctx_destroy(fr_ctx* ctx);
const char* fr_last_error(void);
int fr_default_params(fr_params* out); /* PARAM_MESSAGE_2_CARRY_2, k=1, N=2048 */

/* ----- keys ----- */
/* Randomness.  Every random draw (the client key, the server key's masks and noise, an
 * encryption's masks and noise) is ChaCha20 under one 256-bit generator key.  The *_keyed
 * entry points take it as `const uint8_t* key`: 32 bytes (the 8 little-endian key words),
 * or NULL for 32 fresh bytes of the OS CSPRNG (getrandom(2)) per call, as the reference
 * draws (ciphertext.rs:32-45, engine.rs:252); FR_ERR_RNG if the OS gives none, never a
 * weaker source.  Production callers pass NULL.  A caller-supplied key must be secret,
 * uniform and used for one call: two encryptions under one key share masks and noise
 * block by block, and their difference exposes the plaintexts' difference.
 * The entry points taking `uint64_t seed` run the same generator under the key
 * (seed lo, seed hi, six fixed words).  They exist for tests, benchmarks and reproducible
 * multi-rank keygen: a seed is at most 64 bits and usually known.  Whoever holds a
 * server key and can guess its seed recomputes its noise and solves for the client key,
 * so a server key generated from a known or guessable seed must never leave the client
 * (fr_export_server_key -> fr_load_server_key).
 * A compact server key (fr_gen_server_key_compact*) splits the two uses of the key K of
 * its call: the masks are ChaCha20 words of a mask key, words 0..7 of block 0 of K's
 * stream 8, and the noise stays under K.  The mask key is public by design: it travels in
 * the blob, and the block function is a PRF, so it says nothing about K's other streams.
 * No secret touches a mask word.  The seed caveat stands: the noise of a compact key from
 * a guessable seed is as recomputable as a standard key's, so it must not leave the client. */
/* bincode RadixClientKey (tfhe-rs 0.2 layout, reference test_data/client_key). */
int fr_load_client_key(fr_ctx* ctx, const uint8_t* bincode, size_t len);
/* A fresh client key (gen_keys_radix(&PARAM_MESSAGE_2_CARRY_2, 4), ciphertext.rs:44):
 * uniform binary GLWE key (k*N bits, flattened: the big LWE key) and LWE key (n bits)
 * drawn from a ChaCha20 stream of `seed` (the reference draws from the OS CSPRNG; a seed
 * makes the key reproducible), the parameter block of the context's params.  Replaces
 * any loaded client key and drops the server key.  For tests, benchmarks and reproducible
 * multi-rank keygen: the key has the seed's 64 bits of entropy at most. */
int fr_gen_client_key(fr_ctx* ctx, uint64_t seed);
/* The same key generation under a 256-bit generator key (32 bytes), or under the OS
 * CSPRNG (key == NULL): what gen_keys_radix does. */
int fr_gen_client_key_keyed(fr_ctx* ctx, const uint8_t* key);
/* bincode of the context's client key in the layout fr_load_client_key reads
 * (engine.rs:238-246 generate_test_keys): for a loaded key, the loaded bytes exactly.
 * buf == NULL: size query (*written = bytes needed). */
int fr_serialize_client_key(fr_ctx* ctx, uint8_t* buf, size_t cap, size_t* written);
/* Deterministic server key (KSK mod 2^64; BSK on the 2^64 torus for the FFT
 * ring, mod Q for the RNS ring) from the client key and a seed
 * (ServerKey::new, engine.rs:252; gen_keys_radix, ciphertext.rs:44).  With a
 * device and the FFT ring it is generated on the GPU (FR_KEYGEN_AUTO); the
 * host generator gives the same words bit for bit (fr_set_keygen).  For tests,
 * benchmarks and reproducible multi-rank keygen: a server key generated from a known or
 * guessable seed must never leave the client (see "Randomness" above). */
int fr_gen_server_key(fr_ctx* ctx, uint64_t seed);
/* The same server key generation (same preconditions, same fr_set_keygen placement)
 * under a 256-bit generator key (32 bytes), or under the OS CSPRNG (key == NULL): the
 * one to use for a server key that is exported. */
int fr_gen_server_key_keyed(fr_ctx* ctx, const uint8_t* key);
enum { FR_KEYGEN_AUTO = 0, FR_KEYGEN_HOST = 1, FR_KEYGEN_DEVICE = 2 };
int fr_set_keygen(fr_ctx* ctx, int32_t where);
/* Export the server key: ksk = kN*ks_level*(n+1) u64 ; bsk = W*(k+1)^2*N u64
 * (coefficient domain, torus 2^64 (FFT ring) or mod Q = 998244353*1004535809
 * (RNS ring), layout [w][row][component][coef]).
 * k = 1 or the FFT ring: bootstrapping-key unrolling, W = 3*ceil(n/2) GGSWs,
 * w = 3t+g encrypts s_2t*s_2t+1, s_2t*(1-s_2t+1), (1-s_2t)*s_2t+1 for g = 0, 1, 2;
 * RNS ring with k > 1: W = n, GGSW w encrypts s_w.  Sizes from
 * fr_server_key_sizes.  Either may be NULL. */
int fr_export_server_key(fr_ctx* ctx, uint64_t* ksk, size_t ksk_len, uint64_t* bsk, size_t bsk_len);
int fr_server_key_sizes(fr_ctx* ctx, size_t* ksk_len, size_t* bsk_len);
/* Install a server key in fr_export_server_key's layout: a server context that
 * holds only `sk`, as has_match(sk, content, pattern) takes it (engine.rs:8), never
 * the client key (the reference keeps both in one process: gen_keys, ciphertext.rs:42-45;
 * ServerKey::new, engine.rs:252).  Needs no client key; any client key stays.  The
 * device transforms the BSK into its ring's domain as after fr_gen_server_key.  Lengths
 * other than fr_server_key_sizes' -> FR_ERR_INVALID.  This is the build's own layout,
 * not tfhe-rs's bincode ServerKey. */
int fr_load_server_key(fr_ctx* ctx, const uint64_t* ksk, size_t ksk_len, const uint64_t* bsk, size_t bsk_len);
/* Compact (seeded) server key, FFT ring (FR_RING_RNS -> FR_ERR_INVALID).  A server key in
 * the layouts above whose mask words are all ChaCha20 words of a public 32-byte mask key
 * (see "Randomness"), so that only the bodies and the mask key travel: 3.7x (k = 1,
 * N = 2048) and 5.2x (k = 2, N = 1024) fewer bytes than fr_export_server_key's arrays.
 * KSK mask word row*n + t is u64 number row*n + t of stream 1 under the mask key, BSK mask
 * polynomial j of row (w, r) u64 numbers ((w(k+1) + r)k + j)N + t of stream 3: the
 * standard generator's indices.  The gadget term m_w * 2^(64 - pbs_base_log) that the
 * standard form adds to coefficient 0 of mask polynomial r (rows r < k) would make that
 * word differ from its ChaCha word by a secret, so here it sits in the body:
 * B = sum_j A_j S_j + e - m_w g S_r for r < k, B = sum_j A_j S_j + e + m_w g for r = k.
 * Every row has the phase of the standard form, and every kernel runs on it unchanged.
 * Same preconditions and fr_set_keygen placement as fr_gen_server_key[_keyed]; host and
 * device give the same words.  The installed key is a full server key:
 * fr_export_server_key returns it expanded, valid for fr_load_server_key. */
int fr_gen_server_key_compact(fr_ctx* ctx, uint64_t seed);
int fr_gen_server_key_compact_keyed(fr_ctx* ctx, const uint8_t* key /* NULL: OS CSPRNG */);
/* The wire blob, little endian, exactly fr_server_key_compact_size bytes
 * = 72 + 8*(kN*ks_level + W*(k+1)*N):
 *   bytes 0-7    ASCII "FRCSKEY1"
 *   bytes 8-39   eight int32: k, N, n, ks_base_log, ks_level, pbs_base_log, pbs_level, ring
 *   bytes 40-71  the mask key (8 words)
 *   bytes 72...  KSK bodies [kN*ks_level] u64, then BSK bodies [W][k+1][N] u64
 * fr_export_server_key_compact: buf == NULL is a size query (*written = bytes needed).
 * FR_ERR_NO_KEY without a server key; FR_ERR_INVALID if the installed key was not
 * generated compact or loaded from a blob (a standard key's masks are not expandable
 * from a mask key). */
int fr_server_key_compact_size(fr_ctx* ctx, size_t* bytes);
int fr_export_server_key_compact(fr_ctx* ctx, uint8_t* buf, size_t cap, size_t* written);
/* Install a compact server key: needs no client key, any client key stays.  The length,
 * the magic and all eight integers are checked against the context's params before the
 * installed key is touched; anything else -> FR_ERR_INVALID and the context keeps the key
 * it had.  A device context uploads the bodies only, expands the masks on the GPU and
 * transforms the key there; a host-only context expands on the host.  The context can
 * then export both forms. */
int fr_load_server_key_compact(fr_ctx* ctx, const uint8_t* blob, size_t len);

/* ----- packed results (DESIGN.md §1 "Packed results") -----
 * A packing key is an optional key beside the server key: with it the server puts up to N
 * result booleans into the N coefficients of ONE GLWE ciphertext under the client's own
 * key, (k+1)*N words (32,768 bytes at (k, N) = (1, 2048), 24,576 at (2, 1024)) whether it
 * carries one boolean or N, where every boolean alone is a (kN+1)-word LWE of 16,392 bytes.
 * Nothing else depends on the key's presence.
 * Gadget: signed base 2^7, 3 levels.  Row 3*i + l (i < kN, l < 3) is a GLWE encryption,
 * under the GLWE key (the big key read as k polynomials) with the GLWE noise, of the
 * constant polynomial s_big[i] * 2^(64 - 7*(l+1)): k mask polynomials, then the body;
 * 3*kN = 6,144 rows of (k+1)*N words: 201,326,592 bytes at (1, 2048), 150,994,944 at
 * (2, 1024).  The key encrypts bits of the big key under the big key, a key cycle of the kind the KSK/BSK pair
 * already assumes.  Masks are ChaCha20 words of stream 9, the noise of stream 10, of the
 * generator key.  A device context generates the key on the GPU (fr_set_keygen rules), word
 * for word the host generator's rows; FR_ERR_NO_KEY without a client key.
 * The wire blob, little endian, exactly fr_packing_key_size bytes:
 *     0  "FRPKKEY1"
 *     8  int32 k, N, n, ks_base_log, ks_level, pbs_base_log, pbs_level, ring
 *    40  int32 7, 3 (the packing gadget)
 *    48  the rows
 * fr_export_packing_key: buf == NULL is a size query.  fr_load_packing_key checks the
 * length, the magic, the parameters and the gadget before the installed key is touched
 * (anything else -> FR_ERR_INVALID, the context keeps the key it had), needs no client
 * key, and on a device context first waits for every queued launch. */
int fr_gen_packing_key(fr_ctx* ctx, uint64_t seed);
int fr_gen_packing_key_keyed(fr_ctx* ctx, const uint8_t* key /* NULL: OS CSPRNG */);
int fr_packing_key_size(fr_ctx* ctx, size_t* bytes);
int fr_export_packing_key(fr_ctx* ctx, uint8_t* buf, size_t cap, size_t* written);
int fr_load_packing_key(fr_ctx* ctx, const uint8_t* blob, size_t len);
/* Compact (seeded) packing key, every ring: 3.2x (k = 1, N = 2048) and 4.8x (k = 2, N = 1024)
 * fewer bytes than the blob above.  K is the call's secret generator key and M the public
 * mask key of "Randomness" (words 0..7 of block 0 of K's stream 8, as for a compact server
 * key).  Mask word t of polynomial j of row r is u64 number (r*k + j)*N + t of stream 9 under
 * M: the standard generator's index under another key.  The message sits on the body's
 * coefficient 0, so no mask word carries a secret.  The noise is the standard generator's
 * under K (stream 10).  The body B = sum_j A_j S_j + e + s_big[i] * 2^(64 - 7*(l+1)) on
 * coefficient 0 travels rounded to 40 bits, b40 = ((B + 2^23) >> 24) mod 2^40, and is
 * installed as b40 << 24 on the client as on the server: installed - B lies in
 * (-2^23, 2^23], a 2^-16 share of the variance of the gadget's own rounding.
 * The rounding is a public function of a public ciphertext.  What is installed is an ordinary
 * packing key: every entry above and every packing kernel runs on it unchanged.  Same
 * preconditions and fr_set_keygen placement as fr_gen_packing_key[_keyed]; host and device
 * give the same words.  A compact key from a guessable seed must never leave the client
 * (see "Randomness").
 * The wire blob, little endian, exactly fr_packing_key_compact_size bytes = 96 + 5*3kN*N
 * (62,914,656 at (1, 2048), 31,457,376 at (2, 1024)):
 *     0  "FRCPKEY1"
 *     8  int32 k, N, n, ks_base_log, ks_level, pbs_base_log, pbs_level, ring
 *    40  int32 7, 3 (the packing gadget), int32 40 (body bits), int32 0 (reserved)
 *    56  the mask key M (8 words)
 *    88  8 zero bytes (both planes start 16-byte aligned)
 *    96  high plane u32[3kN][N]: b40 >> 8
 *    96 + 4*3kN*N  low plane u8[3kN][N]: b40 & 0xFF
 * fr_export_packing_key_compact: buf == NULL is a size query; FR_ERR_INVALID without a
 * packing key, or if the installed one was not generated compact or loaded from a compact
 * blob (a standard key's masks are not expandable from a mask key).  A device context
 * gathers the planes on the GPU and downloads them alone.  fr_load_packing_key_compact
 * refuses a wrong length or magic, any of the eight parameters differing from the context's,
 * another gadget, body bits other than 40 and a non-zero reserved word or pad with
 * FR_ERR_INVALID, before the installed key is touched and before anything is allocated; it
 * needs no client key.  A device context uploads the planes in one copy and rebuilds masks
 * and bodies in one kernel; a host-only context expands on the host.  Every other install of
 * a packing key makes the compact export refuse again. */
int fr_gen_packing_key_compact(fr_ctx* ctx, uint64_t seed);
int fr_gen_packing_key_compact_keyed(fr_ctx* ctx, const uint8_t* key /* NULL: OS CSPRNG */);
int fr_packing_key_compact_size(fr_ctx* ctx, size_t* bytes);
int fr_export_packing_key_compact(fr_ctx* ctx, uint8_t* buf, size_t cap, size_t* written);
int fr_load_packing_key_compact(fr_ctx* ctx, const uint8_t* blob, size_t len);
/* The packing keyswitch of n boolean handles (1 <= n <= N): out_words receives the (k+1)*N
 * words of
 *     sum_j X^j * ((0, .., 0, b_j) - sum_{i,l} d_{j,i,l} * row[3*i + l])
 * over (Z_2^64[X]/(X^N+1))^(k+1), d the signed base-2^7 digits of boolean j's mask rounded
 * to 21 bits: coefficient j of its phase is boolean j's phase plus the keyswitch error,
 * coefficients j >= n are that error alone.  Exact integer arithmetic: the device (int8
 * MFMA) and the host compute the same words.  A handle that is no boolean, n outside
 * 1..N or a context without a packing key -> FR_ERR_INVALID.  A host-only context packs
 * trivial booleans only (it has no others).  The call runs after whatever produced the
 * handles and returns after the download.  With fr_set_lanes it runs on lane 0's stream,
 * which first waits for every lane's queued work: packs of results from different lanes
 * are correct but run one after the other, behind all lanes.
 * fr_pack_bools_blob writes the wire blob, exactly fr_packed_result_size bytes:
 *     0  "FRPKRES1"
 *     8  int32 k, N
 *    16  u64 n
 *    24  the (k+1)*N words
 * (buf == NULL: size query).  fr_decrypt_packed (client key needed) refuses a blob of another
 * length, magic, k, N or n outside 1..N with FR_ERR_INVALID before anything is allocated;
 * bits[j] = round(phase_j / 2^59) & 1 for j < n (bits == NULL: *n only); FR_ERR_INVALID if a
 * coefficient j >= n does not round to 0. */
int fr_packed_result_size(fr_ctx* ctx, size_t n, size_t* bytes);
int fr_pack_bools(fr_ctx* ctx, const fr_ct* bools, size_t n, uint64_t* out_words);
int fr_pack_bools_blob(fr_ctx* ctx, const fr_ct* bools, size_t n, uint8_t* buf, size_t cap, size_t* written);
int fr_decrypt_packed(fr_ctx* ctx, const uint8_t* blob, size_t len, uint8_t* bits, size_t* n);
/* Compact packed result (DESIGN.md §1 "Compact reply", §7).  A packed boolean is never
 * bootstrapped again, so only the client's rounding at Delta/2 = 2^58 sees its error.  Every
 * coefficient travels rounded to its top 16 bits, v = ((x + 2^47) >> 48) mod 2^16, and is
 * installed as v << 48, mask and body alike; the body coefficients past n carry no boolean and
 * are not sent.  The rounding adds std sqrt((h+1)/12) * 2^48 to the phase (h the key's weight:
 * 2^51.2 at h = 1024).  The wire blob, little endian, exactly fr_packed_compact_size bytes =
 * 32 + 2*(kN + n) (4,640 at n = 256, 8,224 at n = N, 4,130 at n = 1, all at (1, 2048)):
 *     0  "FRCPRES1"
 *     8  int32 k, N
 *    16  u64 n                      (1 <= n <= N)
 *    24  u32 16 (coefficient bits), u32 0 (reserved)
 *    32  u16 mask[k*N]              (the k mask polynomials, rounded)
 *    ..  u16 body[n]                (body coefficients 0..n-1, rounded)
 * fr_pack_bools_compact is fr_pack_bools_blob in this form: a device context rounds on the GPU
 * and downloads the 2*(kN + n) bytes alone; a host-only context packs trivial booleans.
 * fr_compress_packed is the same rounding of (k+1)*N given words on the host, word for word
 * what the device gives (buf == NULL: size query).  fr_expand_packed_compact checks a blob and
 * writes its (k+1)*N words, v << 48 and a zero body past n (words == NULL: *n only).
 * fr_decrypt_packed_compact (client key needed): bits[j] = round(phase_j / 2^59) & 1 of the
 * expanded words for j < n (bits == NULL: *n only); the coefficients past n were not sent, so
 * unlike fr_decrypt_packed there is nothing to check there.  The last two refuse a wrong
 * length, a wrong magic (FRPKRES1 included), another k or N, n outside 1..N, a bit count other
 * than 16 and a non-zero reserved word with FR_ERR_INVALID before anything is allocated. */
int fr_packed_compact_size(fr_ctx* ctx, size_t n, size_t* bytes);
int fr_pack_bools_compact(fr_ctx* ctx, const fr_ct* bools, size_t n, uint8_t* buf, size_t cap, size_t* written);
int fr_compress_packed(fr_ctx* ctx, const uint64_t* words, size_t n, uint8_t* buf, size_t cap, size_t* written);
int fr_expand_packed_compact(fr_ctx* ctx, const uint8_t* blob, size_t len, uint64_t* words, size_t* n);
int fr_decrypt_packed_compact(fr_ctx* ctx, const uint8_t* blob, size_t len, uint8_t* bits, size_t* n);

/* ----- client side (not on the timed path) ----- */
/* Seeded encryption, for tests and benchmarks only: two calls with one seed share their
 * masks and noise block by block (block q of a call draws at index first_block + q). */
int fr_encrypt_str(fr_ctx* ctx, const char* s, size_t len, uint64_t seed, uint64_t* out /* len*4*(kN+1) */);
int fr_encrypt_blocks(fr_ctx* ctx, const uint8_t* msgs, size_t count, uint64_t seed, uint64_t first_block,
                      uint64_t* out /* count*(kN+1) */);
/* The same encryptions under a 256-bit generator key (32 bytes), or under the OS CSPRNG
 * (key == NULL; what encrypt_str / RadixClientKey::encrypt do, ciphertext.rs:32-40).
 * Errors as the seeded calls: FR_ERR_NO_KEY without a client key, FR_ERR_NON_ASCII. */
int fr_encrypt_str_keyed(fr_ctx* ctx, const char* s, size_t len, const uint8_t* key, uint64_t* out /* len*4*(kN+1) */);
int fr_encrypt_blocks_keyed(fr_ctx* ctx, const uint8_t* msgs, size_t count, const uint8_t* key, uint64_t first_block,
                            uint64_t* out /* count*(kN+1) */);
int fr_decrypt_radix(fr_ctx* ctx, const uint64_t* blocks /* 4*(kN+1) */, uint64_t* value);
int fr_decode_block(fr_ctx* ctx, const uint64_t* lwe, uint32_t* msg_and_carry);

/* ----- ciphertext arena ----- */
int fr_upload_radix(fr_ctx* ctx, const uint64_t* blocks /* n*4*(kN+1) */, size_t n, fr_ct* out /* n */);
int fr_upload_bool(fr_ctx* ctx, const uint64_t* lwe /* n*(kN+1) */, size_t n, fr_ct* out);
/* encrypt_str (ciphertext.rs:32-40) on the device, straight into n_chars
 * content handles: the same ciphertext words as fr_encrypt_str (same seed),
 * without the host encryption and the 64 KB-per-char upload.  Seeded: tests and
 * benchmarks only. */
int fr_encrypt_upload_str(fr_ctx* ctx, const char* s, size_t len, uint64_t seed, fr_ct* out /* len */);
/* The same under a 256-bit generator key (32 bytes; the words of fr_encrypt_str_keyed
 * with that key), or under the OS CSPRNG (key == NULL).  The key travels to the kernel as
 * an argument and is never stored in device memory.  FR_ERR_NO_KEY, FR_ERR_NO_DEVICE,
 * FR_ERR_NON_ASCII as the seeded call. */
int fr_encrypt_upload_str_keyed(fr_ctx* ctx, const char* s, size_t len, const uint8_t* key, fr_ct* out /* len */);
/* Compact (seeded) content ciphertexts, both rings.  All but one word of an LWE block is
 * pseudo-random mask, so the client ships the bodies and a public 32-byte mask key and the
 * server rebuilds the masks: 64 + 8*n_blocks bytes instead of 8*(kN+1)*n_blocks (256
 * chars: 8,256 B instead of 16,785,408 B).  With K the call's generator key (see
 * "Randomness"): the mask key M is words 0..7 of block 0 of K's stream 8, as for a compact
 * server key; mask word t of block q is u64 number (first_block + q)*kN + t of stream 5
 * under M (the standard encryptor's indices under another key); the body is
 * <mask, s_big> + m*2^59 + the standard encryptor's noise, which stays under K.  An LWE
 * mask is public in the ordinary form too; no secret touches a mask word.  The keyed
 * calls' caveat stands: two blobs made under one K share masks and noise block by block.
 * The wire blob, little endian, exactly fr_compact_content_size bytes = 64 + 8*n_blocks:
 *   bytes 0-7    ASCII "FRCCTXT1"
 *   bytes 8-15   int32 k, int32 N
 *   bytes 16-23  u64 first_block
 *   bytes 24-31  u64 n_blocks
 *   bytes 32-63  the mask key (8 words)
 *   bytes 64...  n_blocks u64 bodies
 * A blob is refused with FR_ERR_INVALID, before anything is allocated, unless its length
 * is exact, the magic matches, k and N are the context's, first_block + n_blocks <= 2^40
 * and, for fr_upload_compact_str, n_blocks % 4 == 0.
 * Encryption (client): key == NULL draws K from the OS CSPRNG (production), else the
 * caller's 32 bytes; buf == NULL is a size query (*written = bytes needed); FR_ERR_NO_KEY
 * without a client key, FR_ERR_NON_ASCII, FR_ERR_RNG, FR_ERR_INVALID for cap too small. */
int fr_compact_content_size(fr_ctx* ctx, size_t n_blocks, size_t* bytes);
int fr_encrypt_str_compact_keyed(fr_ctx* ctx, const char* s, size_t len, const uint8_t* key, uint8_t* buf, size_t cap,
                                 size_t* written); /* 4 blocks per char, first_block 0 */
int fr_encrypt_blocks_compact_keyed(fr_ctx* ctx, const uint8_t* msgs, size_t count, const uint8_t* key,
                                    uint64_t first_block, uint8_t* buf, size_t cap, size_t* written);
/* Host expansion to the full LWE words; needs no key.  out has room for
 * out_words >= n_blocks*(kN+1) (else FR_ERR_INVALID); out == NULL: *n_blocks only. */
int fr_expand_compact_content(fr_ctx* ctx, const uint8_t* blob, size_t len, uint64_t* out, size_t out_words,
                              size_t* n_blocks);
/* Device expansion straight into fresh arena slots; needs no client key.  The handles are
 * ordinary content: radix handles as fr_upload_radix's (4 blocks per character), boolean
 * handles as fr_upload_bool's (one block each).  Only the bodies and the slot list cross
 * the bus, in one copy; the call returns once the expansion is enqueued on the context's
 * stream, the blob may be freed on return, and every later operation of the context, on
 * any lane, is ordered after it.  *n_chars / *n = handles needed; cap smaller than that,
 * or a bad blob -> FR_ERR_INVALID with no slot or handle left allocated;
 * FR_ERR_NO_DEVICE on a host-only context (after the checks of the blob and of cap). */
int fr_upload_compact_str(fr_ctx* ctx, const uint8_t* blob, size_t len, fr_ct* out, size_t cap, size_t* n_chars);
int fr_upload_compact_blocks(fr_ctx* ctx, const uint8_t* blob, size_t len, fr_ct* out, size_t cap, size_t* n);
/* Wire format of a radix ciphertext: bincode (fixint, little endian) of tfhe-rs
 * 0.2 RadixCiphertext — u64 n_blocks, then per block u64 len (= kN+1), the LWE
 * words, u64 degree, u64 message_modulus (4), u64 carry_modulus (4).  [ext]
 * unverified against tfhe-rs (absent here); follows the conventions of the
 * verified client-key layout (Vec<u64> = u64 length + words, usize = u64).
 * buf == NULL / blocks == NULL: size query only. */
int fr_radix_serialize(fr_ctx* ctx, const uint64_t* blocks, size_t n_blocks, uint64_t degree, uint8_t* buf, size_t cap,
                       size_t* written);
int fr_radix_deserialize(fr_ctx* ctx, const uint8_t* buf, size_t len, uint64_t* blocks, size_t max_blocks,
                         size_t* n_blocks);
int fr_download_radix(fr_ctx* ctx, fr_ct h, uint64_t* out /* 4*(kN+1) */);
int fr_release(fr_ctx* ctx, fr_ct h);
int fr_trivial(fr_ctx* ctx, uint8_t value, fr_ct* out);

/* ----- eager gate ops: one call per reference smart_* call ----- */
int fr_eq_const(fr_ctx* ctx, fr_ct a, uint8_t c, fr_ct* out);
int fr_gt_const(fr_ctx* ctx, fr_ct a, uint8_t c, fr_ct* out);
int fr_le_const(fr_ctx* ctx, fr_ct a, uint8_t c, fr_ct* out);
int fr_and(fr_ctx* ctx, fr_ct a, fr_ct b, fr_ct* out);
int fr_or(fr_ctx* ctx, fr_ct a, fr_ct b, fr_ct* out);
int fr_not(fr_ctx* ctx, fr_ct a, fr_ct* out);
/* OR of n boolean ciphertexts (multi-GPU partial-result reduction). */
int fr_or_many(fr_ctx* ctx, const fr_ct* in, size_t n, fr_ct* out);

/* ----- batched gate program ----- */
/* One programmable bootstrap of s = offset/2 + sum_i w_i * in_i (offset in
 * units of Delta/2; inputs are boolean/radix-block handles, block in_block[i]
 * of in[i]).  kind FR_GATE_LUT: s integral in [0,16), out = lut[s];
 * kind FR_GATE_SIGN: s half-integral in (-16,16), out = [s > 0] (threshold
 * AND/OR of up to 16 booleans). */
enum { FR_GATE_LUT = 0, FR_GATE_SIGN = 1 };
typedef struct {
    int32_t n_in;
    int32_t offset;
    int32_t kind;
    fr_ct in[16];
    int8_t in_block[16];
    int8_t in_w[16];
    uint8_t lut[16];
    fr_ct out; /* filled by fr_run_gates: a fresh boolean handle */
} fr_gate;
/* Runs n gates; a gate may consume the output of an earlier gate in the same
 * call by referencing FR_GATE_REF(j) as its input handle.  Level-scheduled
 * into batched device launches. */
#define FR_GATE_REF(j) (0x80000000u | (uint32_t)(j))
int fr_run_gates(fr_ctx* ctx, fr_gate* gates, size_t n);

/* ----- the engine (engine.rs:8-42) ----- */
/* Enumerate, record, lower and execute has_match over content handles.  The
 * result is a boolean radix handle (decrypts to 0/1).  Pattern errors return
 * FR_ERR_PARSE / FR_ERR_REF_PANIC like the reference.  By default the call returns
 * once the match's launches are enqueued on the context's stream: the result
 * handle can be used at once (every later operation of the context is ordered after
 * the match, and downloads wait for it), so consecutive matches overlap their host
 * work with the device's; fr_set_async(ctx, 0) makes the engine calls block until
 * the device has finished. */
int fr_set_async(fr_ctx* ctx, int32_t on);
/* Lanes (round 5; serving with one key): n >= 2 gives the context's device n more
 * streams ("lanes") beside its own, each with its own keyswitch scratch and content map;
 * consecutive asynchronous
 * matches of a cacheable plan go round-robin over the lanes (each lane its own copy of the
 * plan), so one match's small levels share the chip with the next match's first level.
 * Every other operation runs on lane 0 after the lanes' enqueued work (device-side event
 * waits); results are bit-identical to n = 1.  n = 1 (default): one stream.  1 <= n <= 8. */
int fr_set_lanes(fr_ctx* ctx, int32_t n);
int fr_has_match(fr_ctx* ctx, const fr_ct* content, size_t n_chars, const char* pattern, fr_ct* out,
                 fr_match_stats* stats);
/* Same, restricted to start offsets [start_lo, start_hi) — the per-GPU shard of
 * the start-offset partition (the OR over shards equals has_match). */
int fr_has_match_range(fr_ctx* ctx, const fr_ct* content, size_t n_chars, const char* pattern, size_t start_lo,
                       size_t start_hi, fr_ct* out, fr_match_stats* stats);
/* Same start range, the result as *n_parts <= max_parts booleans out[0..n_parts) whose OR
 * is fr_has_match_range's result (round 5).  The threshold lowering's OR tree over the
 * range's start offsets (engine.rs:22-35) stops once <= max_parts literals remain, so a
 * caller OR-ing the parts of W start shards (W * max_parts <= 16: one threshold OR) spends
 * the tree's last level once instead of once per shard plus once to combine.  Faithful
 * lowerings, and roots that are not an OR, give one part.  1 <= max_parts <= 16; out has
 * room for max_parts handles; each part is a boolean handle of its own. */
int fr_has_match_parts(fr_ctx* ctx, const fr_ct* content, size_t n_chars, const char* pattern, size_t start_lo,
                       size_t start_hi, size_t max_parts, fr_ct* out, size_t* n_parts, fr_match_stats* stats);
/* n_matches independent has_match calls of one pattern over n_matches contents
 * of n_chars each (content[m * n_chars + q], out[m]): the matches' circuits run
 * as one plan, so each dependency level of all matches shares its launches
 * (throughput mode; every out[m] is bit-identical to fr_has_match on content m).
 * stats: ct_ops / cache_hits / n_branches of one match; pbs, blind_rotations of
 * the batch; levels of one match (= of the batch). */
int fr_has_match_batch(fr_ctx* ctx, const fr_ct* content, size_t n_chars, size_t n_matches, const char* pattern,
                       fr_ct* out, fr_match_stats* stats);
/* Plan cache: has_match circuits are data-oblivious, so the lowered, compiled
 * plan of (pattern, grammar, engine, lowering, multi-value, n_chars, batch size,
 * start range, content shape) is kept -- its intermediate slots and its
 * device-resident gate batches -- and a repeat call binds the call's content
 * slots (a content map read by the keyswitch) and enqueues the levels.  The
 * content shape is which blocks are trivial (and their values) and which
 * positions share a ciphertext, not the ciphertexts: fresh content of the same
 * shape hits.  capacity = plans kept (LRU; default 8, env FR_PLAN_CACHE); 0
 * disables and frees every cached plan.  max_slots bounds the intermediate arena
 * slots all cached plans hold ((kN+1) u64 each; default 2^18, env
 * FR_PLAN_CACHE_SLOTS); eviction runs before a new plan allocates, and a plan
 * larger than max_slots runs uncached. */
int fr_set_plan_cache(fr_ctx* ctx, size_t capacity);
int fr_set_plan_cache_slots(fr_ctx* ctx, size_t max_slots);
int fr_plan_cache_stats(fr_ctx* ctx, uint64_t* entries, uint64_t* slots, uint64_t* hits, uint64_t* misses);

/* Booleans (block 0 of each handle) to / from a device buffer of n * (kN+1) u64
 * (the start-offset shards' partial results gathered over RCCL without a host
 * round trip; the reference's final ct_or fold, engine.rs:22-35).  Both
 * synchronise the library's stream before returning. */
int fr_export_bool_device(fr_ctx* ctx, const fr_ct* h, size_t n, uint64_t* dev_dst);
int fr_import_bool_device(fr_ctx* ctx, const uint64_t* dev_src, size_t n, fr_ct* out);
/* Stream-ordered export (n <= 16): enqueued on the library's stream (fr_stream) after
 * every earlier operation of the context, returns without synchronising; a caller
 * orders its own stream after it with an event (e.g. the RCCL all-gather of the
 * start-offset shards, which then never blocks the host between matches).  Handles
 * with a trivial block 0 take the synchronising path. */
int fr_export_bool_device_async(fr_ctx* ctx, const fr_ct* h, size_t n, uint64_t* dev_dst);
/* The context's HIP stream (hipStream_t): every device operation of the context is
 * ordered on it. */
int fr_stream(fr_ctx* ctx, void** stream);
/* Accumulated kernel timers of the profiling mode (fr_set_profiling): blind
 * rotation and (level 2) keyswitch milliseconds, launches and bootstraps. */
int fr_device_timers(fr_ctx* ctx, double* br_ms, double* ks_ms, uint64_t* br_launches, uint64_t* br_gates);
/* The part of those blind-rotation timers spent in latency-shape launches (at
 * most one bootstrap per CU: one workgroup per CU). */
int fr_device_timers_latency(fr_ctx* ctx, double* br_ms, uint64_t* br_launches, uint64_t* br_gates);
/* ... and in pair-shape launches (FFT ring, k = 1: two bootstraps per workgroup in the
 * latency geometry, for batches above the latency shape's limit). */
int fr_device_timers_pair(fr_ctx* ctx, double* br_ms, uint64_t* br_launches, uint64_t* br_gates);
/* The stages of the last fr_load_server_key_compact made under fr_set_profiling, by HIP
 * events: ms[0..4] = H2D copy of the bodies, KSK mask expansion, BSK mask expansion, KSK
 * byte limbs, Fourier transform of the BSK. */
int fr_device_timers_key_load(fr_ctx* ctx, double* ms /* 5 */);
/* The same for the last fr_load_packing_key_compact: ms[0..2] = H2D copy of the planes, the
 * expansion kernel (masks and bodies), the byte limbs. */
int fr_device_timers_packing_key_load(fr_ctx* ctx, double* ms /* 3 */);
/* The expansion kernel of the last fr_upload_compact_* made under fr_set_profiling, by HIP
 * events, ms.  A profiled upload waits for its kernel; an unprofiled one does not. */
int fr_device_timers_content(fr_ctx* ctx, double* ms);
/* The stages of the last fr_pack_bools made under fr_set_profiling, by HIP events:
 * ms[0..2] = digits (with the zeroing of the scratch), int8 GEMM, rotate-and-sum. */
int fr_device_timers_pack(fr_ctx* ctx, double* ms /* 3 */);
/* The same three stages and ms[3], the compact form's rounding kernel (0 after a pack in the
 * full form), of the last pack of either form, fr_match_starts_packed's included. */
int fr_device_timers_pack_compact(fr_ctx* ctx, double* ms /* 4 */);

/* Match starts: where the pattern matches, not only whether.  out[s - start_lo] is a boolean
 * handle that decrypts to whether the pattern matches starting at offset s, for every s of
 * [start_lo, start_hi): the value the reference ORs away at engine.rs:22-35, i.e.
 * has_match restricted to the starts [s, s + 1).  One program for all starts: the per-start
 * programs merged, a gate with the inputs, offset, kind and table of an earlier one being
 * that gate, so the nibble tests of a character are shared by every start that reads it.  A
 * start whose value is a constant (/^abc/ at s > 0) gives a trivial boolean.  Errors, the
 * plan cache, lanes and fr_set_async as fr_has_match_range.  fr_pack_bools puts the handles
 * into one reply. */
int fr_match_starts(fr_ctx* ctx, const fr_ct* content, size_t n_chars, const char* pattern, size_t start_lo,
                    size_t start_hi, fr_ct* out /* start_hi - start_lo */, fr_match_stats* stats);
/* From match to reply in one call: fr_match_starts' booleans of [start_lo, start_hi),
 * 1 <= start_hi - start_lo <= N, packed into one blob, compact = 0 the FRPKRES1 form and 1 the
 * FRCPRES1 form, byte for byte what fr_match_starts + fr_pack_bools_blob (then
 * fr_compress_packed) give.  The plan is fr_match_starts' own: one compiled by either call
 * serves the other.  Each start's affine output is read by the packing keyswitch straight
 * from the plan's gate slot: no handle, no arena slot and no launch per start.  With
 * fr_set_lanes the pack runs on the match's own lane after the plan's launches, on that lane's
 * scratch; the call returns after its own download and waits for no other lane, so replies of
 * matches on different lanes overlap (after fr_set_async(0) it then waits for every lane, as
 * every blocking match does).  buf == NULL: size query.  FR_ERR_INVALID without a
 * packing key, before anything is launched; other errors as fr_match_starts. */
int fr_match_starts_packed(fr_ctx* ctx, const fr_ct* content, size_t n_chars, const char* pattern, size_t start_lo,
                           size_t start_hi, int32_t compact, uint8_t* buf, size_t cap, size_t* written,
                           fr_match_stats* stats);

/* ----- private search: an encrypted needle on encrypted content (FFT ring) ----- */
/* Every match entry above takes its pattern in the clear.  A needle is the encrypted form of a
 * fixed-length query: character i is a product class lo_mask x hi_mask of accepted low and high
 * nibble values (16-bit masks; a literal byte: one bit in each; a case-insensitive letter: two
 * bits in the high mask; any byte: 0xFFFF, 0xFFFF).  The client encrypts each of the 2 m masks
 * as a selector, a GLWE ciphertext of (k+1) N words under its GLWE key whose phase is the
 * direct test polynomial of the mask read as a 0/1 table; selector 2 i + h tests nibble h
 * (0: low) of character i.  The server starts one blind rotation per (content nibble, needle
 * nibble) from the selector instead of from a table of its own, so it learns the needle's length
 * m and the content length, and nothing else about the query.
 * Blob: "FRNEEDL1", int32 k, N, u64 m, the 32-byte public mask key, 8 zero bytes, then the 2 m
 * body polynomials of N u64; little endian, exactly 64 + 16 m N bytes (fr_needle_size; 32 KB per
 * character at (1, 2048)).  Mask word t of mask polynomial c of selector q is u64 number
 * (q k + c) N + t of ChaCha20 stream 11 under the mask key; the noise (GLWE sigma) is drawn
 * under the call's secret key.  1 <= m <= 64.
 * fr_encrypt_needle_keyed (client key needed): masks[2 i], masks[2 i + 1] = lo, hi of character
 * i; key NULL: the OS CSPRNG; buf NULL: size query.  fr_expand_needle (no key needed): the
 * 2 m (k+1) N words [selector][polynomial][N]; words NULL: *m only.  Both refuse an RNS context,
 * and every blob whose length, magic, k, N, m or pad is off, with FR_ERR_INVALID before anything
 * is allocated. */
int fr_needle_size(fr_ctx* ctx, size_t m, size_t* bytes);
int fr_encrypt_needle_keyed(fr_ctx* ctx, const uint16_t* masks /* 2*m: lo, hi per character */, size_t m,
                            const uint8_t* key /* NULL: OS CSPRNG */, uint8_t* buf, size_t cap, size_t* written);
int fr_expand_needle(fr_ctx* ctx, const uint8_t* blob, size_t len, uint64_t* words, size_t cap_words, size_t* m);
/* Server side (needs no client key): the blob expanded on the host and sent in one H2D copy.  The
 * needle belongs to the context's device; fr_needle_free first waits for every lane, as a cached
 * plan's release does, so it may follow asynchronous finds directly.  Free every needle of a
 * context before fr_ctx_destroy: a needle that outlives its context must not be freed or used.
 * fr_needle_free takes the context the needle was uploaded to (another: FR_ERR_INVALID, nothing
 * freed); a NULL needle is no error. */
typedef struct fr_needle fr_needle;
int fr_upload_needle(fr_ctx* ctx, const uint8_t* blob, size_t len, fr_needle** out);
int fr_needle_len(const fr_needle* needle, size_t* m);
int fr_needle_free(fr_ctx* ctx, fr_needle* needle);
/* fr_find: out = [the needle matches at some start p of [start_lo, start_hi) with p + m <= n_chars],
 * the OR a has_match of the same literal gives.  fr_find_starts: out[p - start_lo] = [it matches at
 * p], start_hi - start_lo booleans; a start that cannot fit the needle is a trivial 0, as
 * fr_match_starts gives (at most 2^24 starts a call).  m > n_chars is no error: the constant.
 * fr_find reads only the starts that fit, whatever start_hi.  Both run through the match
 * engine: plan cache (the plan depends on m and the content's shape, never on the needle's
 * ciphertext: a second needle of the same length is a hit), lanes, fr_set_async, stats.  Cost: one
 * rotation per (content nibble, needle nibble) and start, then the AND per start and the OR.
 * FR_ERR_INVALID for an RNS context, a needle of another (k, N) or of another context;
 * FR_ERR_NO_DEVICE on a host-only context; nothing is launched then. */
int fr_find(fr_ctx* ctx, const fr_ct* content, size_t n_chars, const fr_needle* needle, size_t start_lo,
            size_t start_hi, fr_ct* out, fr_match_stats* stats);
int fr_find_starts(fr_ctx* ctx, const fr_ct* content, size_t n_chars, const fr_needle* needle, size_t start_lo,
                   size_t start_hi, fr_ct* out /* start_hi - start_lo */, fr_match_stats* stats);

/* ----- private search over clear content (FFT ring) ----- */
/* The same search where the server holds the text itself (a corpus, a log, a mailbox it hosts)
 * and only the needle is encrypted: fr_find_clear and fr_find_clear_starts give fr_find's and
 * fr_find_starts' booleans for the n_chars bytes at `content` (a pointer and a length: every byte
 * value is valid, 0x00 and bytes >= 0x80 included; copied before the call returns).  A blind
 * rotation by a known nibble v is the monomial X^(-v N/16), so the first level needs no rotation:
 * bit v of selector q's table is coefficient v N/16 of its phase, and the sample extract there
 * is an LWE of that bit under the flattened GLWE key, with the selector's fresh noise alone.
 * Extraction is linear, so the sum the per-start AND reads is formed straight from the needle's
 * table by one kernel, one big LWE per gate (none per content nibble), and a find costs one
 * rotation per start that fits for m <= 8 (two levels of them above that), plus fr_find_clear's
 * OR tree.  The server learns m; the client learns the booleans.  Circuit privacy of the reply is
 * not claimed: the outputs are bootstrap outputs, their noise the server key's, as every match's.
 * Both run through the match engine: plan cache (the plan depends on m, n_chars and the range,
 * never on the bytes or on the needle's ciphertext: a second text of the same length is a hit, and
 * so is a second needle of the same length; fr_find's plans are kept apart), lanes, fr_set_async,
 * stats (pbs and blind_rotations count rotations only).  The bytes travel per call, in stream
 * order on the match's lane.  m > n_chars is no error: the constant; a start that cannot fit is
 * a trivial 0.  FR_ERR_INVALID for an RNS context, a needle of another (k, N) or of another
 * context, a NULL content with n_chars > 0, start_lo > start_hi; FR_ERR_NO_DEVICE on a host-only
 * context; nothing is launched then. */
int fr_find_clear(fr_ctx* ctx, const uint8_t* content, size_t n_chars, const fr_needle* needle, size_t start_lo,
                  size_t start_hi, fr_ct* out, fr_match_stats* stats);
int fr_find_clear_starts(fr_ctx* ctx, const uint8_t* content, size_t n_chars, const fr_needle* needle,
                         size_t start_lo, size_t start_hi, fr_ct* out /* start_hi - start_lo */,
                         fr_match_stats* stats);

/* ----- scan of a long clear text (FFT ring) ----- */
/* fr_find_clear spends one rotation per start; a start's result depends only on the m bytes of
 * its window, and the server knows the text, so a scan spends one rotation per *distinct window*.
 * The starts of the range are classed on the host (fr_window_classes), the distinct windows are
 * laid side by side, their count D padded to the next multiple of 64 by repeating window 0
 * (harmless in an OR, read by no start; texts with nearby D share one plan), and the search runs
 * over the windows alone: the plan depends on (m, padded D) and never on the bytes, so a second
 * text or needle of the same (m, padded D) is a cache hit; its plans are kept apart from
 * fr_find_clear's.  fr_scan_clear is fr_find_clear's boolean.  fr_scan_clear_starts is
 * fr_find_clear_starts followed by the packs of its handles, without the handles: buf receives the
 * blobs of the ceil((start_hi - start_lo) / N) chunks of N starts back to back, FRPKRES1
 * (compact = 0) or FRCPRES1 (1), chunk c carrying starts start_lo + c N onward in order, byte for
 * byte what fr_pack_bools_blob / fr_pack_bools_compact give for fr_find_clear_starts' handles.
 * One plan launch serves every chunk; per chunk the packing keyswitch runs over the classes that
 * occur in it and start j of class d is X^j times row d (linearity), on the match's lane after
 * the plan's launches.  A start that cannot fit, or lies past the content, is the constant 0.
 * *written receives the reply's size; buf NULL is a size query; cap too small is FR_ERR_INVALID
 * with *written set and nothing launched.  Stats count rotations as every match's (host_ms
 * includes the classing);
 * fr_scan_classes gives D and padded D of the context's last scan.  Limits: n_chars <= 2^24,
 * start_hi - start_lo <= 2^24, padded D times m <= 2^24.  Refusals, lanes, fr_set_async and the
 * needle's release are fr_find_clear's; fr_scan_clear_starts needs the packing key. */
int fr_scan_clear(fr_ctx* ctx, const uint8_t* content, size_t n_chars, const fr_needle* needle, size_t start_lo,
                  size_t start_hi, fr_ct* out, fr_match_stats* stats);
int fr_scan_clear_starts(fr_ctx* ctx, const uint8_t* content, size_t n_chars, const fr_needle* needle,
                         size_t start_lo, size_t start_hi, int32_t compact, uint8_t* buf, size_t cap, size_t* written,
                         fr_match_stats* stats);
int fr_scan_classes(fr_ctx* ctx, uint64_t* classes, uint64_t* padded);

/* ----- byte-table needles: per-position byte classes over clear content (FFT ring) ----- */
/* Over clear content no rotation touches the needle: the extract-sum reads one coefficient the
 * server computes from a byte it knows, and that is exact at any coefficient.  A byte-table needle
 * therefore carries one 0/1 table of the 256 byte values per character -- any class, [0-9], [^x],
 * \w, not only a product lo_mask x hi_mask -- and N/256 tables share one selector: the phase of
 * coefficient (i % (N/256)) 256 + b of selector i / (N/256) is T_i[b] 2^59, with no boxes, no
 * recentring and no negacyclic sign; coefficients past the last table encrypt 0.  A start's AND
 * reads m terms instead of 2 m: one rotation per start up to m = 16.
 * Blob: "FRNEEDB1", int32 k, N, u64 m, the 32-byte public mask key, 8 zero bytes, then the
 * G = ceil(256 m / N) body polynomials of N u64; little endian, exactly 64 + 8 G N bytes
 * (fr_needle_bytes_size; 16,448 bytes for m = 8 at (1, 2048)).  Mask word t of mask polynomial c
 * of selector q is u64 number (q k + c) N + t of ChaCha20 stream 13 under the mask key; the noise
 * (GLWE sigma) is drawn from stream 14 under the call's secret key.  1 <= m <= 64.  The server
 * learns m: literal, class, case-insensitive and wildcard positions look alike.
 * fr_encrypt_needle_bytes_keyed (client key needed): 32 bytes per character, bit b of table i =
 * tables[32 i + b / 8] >> (b % 8) & 1; key and size query as fr_encrypt_needle_keyed.
 * fr_expand_needle_bytes (no key needed): the G (k+1) N words [selector][polynomial][N]; words
 * NULL: *m only.  Refusals as the nibble needle's, before anything is allocated.
 * fr_upload_needle takes either blob (told apart by the magic) and the needle remembers its form
 * (fr_needle_form).  fr_find_clear, fr_find_clear_starts, fr_scan_clear and fr_scan_clear_starts
 * accept either form; their plans are kept apart by form.  fr_find and fr_find_starts refuse a
 * byte-table needle with FR_ERR_INVALID before anything is launched: those searches need rotations
 * of the needle's tables, which only the nibble form allows. */
enum { FR_NEEDLE_NIBBLES = 0, FR_NEEDLE_BYTES = 1 };
int fr_needle_bytes_size(fr_ctx* ctx, size_t m, size_t* bytes);
int fr_encrypt_needle_bytes_keyed(fr_ctx* ctx, const uint8_t* tables /* 32 per character */, size_t m,
                                  const uint8_t* key /* NULL: OS CSPRNG */, uint8_t* buf, size_t cap, size_t* written);
int fr_expand_needle_bytes(fr_ctx* ctx, const uint8_t* blob, size_t len, uint64_t* words, size_t cap_words, size_t* m);
int fr_needle_form(const fr_needle* needle, int32_t* form);
/* The classing alone, on the host: for the starts p of [start_lo, min(start_hi, n_chars)),
 * cls[p - start_lo] is the index of p's window text[p .. p + m) among the distinct windows in order
 * of first appearance, or -1 where p + m > n_chars; *n_cls entries are written (cls NULL: none).
 * *classes is D, *padded the plan's count, and windows (NULL: skipped) receives the D windows side
 * by side, D m bytes.  Windows are compared byte for byte; every byte value is valid. */
int fr_window_classes(const uint8_t* text, size_t n_chars, size_t m, size_t start_lo, size_t start_hi, int32_t* cls,
                      size_t cls_cap, size_t* n_cls, uint64_t* classes, uint64_t* padded, uint8_t* windows,
                      size_t windows_cap);

/* ----- one match split across ranks ----- */
/* The reference folds ct_or over the branches of every start offset
 * (engine.rs:15-35, each branch a chain of execution.rs:76-190 calls); anchored
 * patterns have one start (engine.rs:51-57), so start offsets alone do not
 * spread their work.  A shard plan splits every dependency level of the lowered
 * circuit instead: each rank compiles the same plan over its copy of the
 * content (same pattern, content length and start range on every rank), runs a
 * contiguous slice [begin, end) of each level's rotation jobs, exports the
 * slice's output LWEs (kN+1 u64 each, job order) into a device buffer, and after
 * an all-gather imports the other ranks' slices; the last level's output then
 * exists on the ranks that hold it (fr_shard_finish).  Levels are 0-based.
 * export / import synchronise the library's stream before returning; the
 * caller orders its own stream (the all-gather) around them.  The plan reads the
 * content handles' arena slots as they were at fr_shard_plan: the content must
 * stay alive (not fr_release'd) until fr_shard_free.  fr_shard_plan merges
 * same-input gates by arena slot, so its levels equal fr_schedule_match's only
 * when every content handle is distinct and encrypted (fheregex.closure_parts
 * checks that the two agree). */
typedef struct fr_shard fr_shard;
int fr_shard_plan(fr_ctx* ctx, const fr_ct* content, size_t n_chars, const char* pattern, size_t start_lo,
                  size_t start_hi, fr_shard** out, fr_match_stats* stats);
int fr_shard_levels(const fr_shard* sh, uint32_t* levels);
int fr_shard_jobs(const fr_shard* sh, uint32_t level, uint32_t* jobs);
int fr_shard_outputs(const fr_shard* sh, uint32_t level, uint32_t begin, uint32_t end, uint32_t* n_lwe);
int fr_shard_run(fr_ctx* ctx, fr_shard* sh, uint32_t level, uint32_t begin, uint32_t end); /* async */
int fr_shard_export(fr_ctx* ctx, fr_shard* sh, uint32_t level, uint32_t begin, uint32_t end, uint64_t* dev_dst);
int fr_shard_import(fr_ctx* ctx, fr_shard* sh, uint32_t level, uint32_t begin, uint32_t end, const uint64_t* dev_src);
/* boolean result handle (valid on a rank that ran or imported the last level) */
int fr_shard_finish(fr_ctx* ctx, fr_shard* sh, fr_ct* out, fr_match_stats* stats);
int fr_shard_free(fr_ctx* ctx, fr_shard* sh);

/* The schedule of such a plan without a device (CPU evaluators, tests): rotation
 * job j of level l is jobs[level_off[l] .. level_off[l+1]); every content
 * position of [0, n_chars) counts as an encrypted radix character.  in_ref[q] >= 0
 * is the output of program gate in_ref[q], in_ref[q] < 0 content block
 * -1 - in_ref[q] (= 4 pos + block, LSB block first); job input s = offset/2 +
 * sum w_q in_q (units of Delta); kind 1: out_gate[0] = lut[0][s]; kind 0
 * (multi-value): out_gate[f] = lut[f][s], f < n_out; kind 2: [s > 0]; kind 3 (private
 * search): out_gate[0] = T[s] for the needle's table T of selector lut[0][0..3] (u32, little
 * endian), which the schedule does not hold.  out3 =
 * (out_gate, out_w, out_const): result = out_const + out_w * gate (out_gate < 0:
 * the constant).  Pass jobs / level_off = NULL to query the sizes. */
typedef struct {
    int32_t n_in;
    int32_t offset;
    int32_t in_ref[16];
    int32_t in_w[16];
    int32_t n_out;
    int32_t kind;
    int32_t out_gate[8];
    uint8_t lut[8][16];
} fr_job;
int fr_schedule_match(size_t n_chars, const char* pattern, size_t start_lo, size_t start_hi, int32_t lowering,
                      int32_t engine, int32_t grammar, int32_t multi_value, fr_job* jobs, size_t jobs_cap,
                      size_t* n_jobs, uint32_t* level_off, size_t level_cap, size_t* n_levels, int32_t* out3);
/* The schedule of fr_has_match_parts' program: outs3[3j .. 3j+2] = part j's (out_gate,
 * out_w, out_const), j < *n_parts (outs3 has room for 3 * max_parts). */
int fr_schedule_match_parts(size_t n_chars, const char* pattern, size_t start_lo, size_t start_hi, int32_t lowering,
                            int32_t engine, int32_t grammar, int32_t multi_value, size_t max_parts, fr_job* jobs,
                            size_t jobs_cap, size_t* n_jobs, uint32_t* level_off, size_t level_cap, size_t* n_levels,
                            int32_t* outs3, size_t* n_parts);

/* fr_schedule_match_parts for the merged program of fr_match_starts: outs3[3*j .. 3*j+2] =
 * (out_gate, out_w, out_const) of start start_lo + j, j < *n_starts = start_hi - start_lo
 * <= outs_cap. */
int fr_schedule_match_starts(size_t n_chars, const char* pattern, size_t start_lo, size_t start_hi, int32_t lowering,
                             int32_t engine, int32_t grammar, int32_t multi_value, fr_job* jobs, size_t jobs_cap,
                             size_t* n_jobs, uint32_t* level_off, size_t level_cap, size_t* n_levels, int32_t* outs3,
                             size_t outs_cap, size_t* n_starts);
/* The schedule of fr_find (starts = 0: one output) or fr_find_starts (starts = 1: one per start
 * of the range) for a needle of m characters: level 1, the first entry of
 * level_off, holds the kind-3 jobs alone. */
int fr_schedule_find(size_t n_chars, size_t m, size_t start_lo, size_t start_hi, int32_t starts, fr_job* jobs,
                     size_t jobs_cap, size_t* n_jobs, uint32_t* level_off, size_t level_cap, size_t* n_levels,
                     int32_t* outs3, size_t outs_cap, size_t* n_outs);
/* The lowered programs of fr_find_starts and fr_find evaluated in plaintext, gate by gate, with
 * the tables in the clear: starts_out[p - start_lo] and *any. */
int fr_plain_find(const char* content, size_t len, const uint16_t* masks, size_t m, size_t start_lo, size_t start_hi,
                  uint8_t* starts_out, int32_t* any);
/* The schedule of fr_find_clear (starts = 0) or fr_find_clear_starts (starts = 1), shaped as
 * fr_schedule_find.  There is no kind-3 job: the extract-sums are level 0, neither jobs nor
 * rotations, and a kind-2 job of level 1 reads one of them as its single input (in_ref[0]: the
 * sum's program gate, in_w[0] = 1), its offset the AND's over the sum's terms. */
int fr_schedule_find_clear(size_t n_chars, size_t m, size_t start_lo, size_t start_hi, int32_t starts, fr_job* jobs,
                           size_t jobs_cap, size_t* n_jobs, uint32_t* level_off, size_t level_cap, size_t* n_levels,
                           int32_t* outs3, size_t outs_cap, size_t* n_outs);
/* The lowered programs of fr_find_clear_starts and fr_find_clear evaluated in plaintext, the
 * extract-sums included, with the tables in the clear: starts_out[p - start_lo] and *any. */
int fr_plain_find_clear(const uint8_t* content, size_t len, const uint16_t* masks, size_t m, size_t start_lo,
                        size_t start_hi, uint8_t* starts_out, int32_t* any);
/* The schedule of fr_scan_clear (starts = 0) or of fr_scan_clear_starts' plan (starts = 1) over
 * n_windows windows of m bytes, shaped as fr_schedule_find_clear: window d's extract-sum terms
 * read the compacted text from byte d m on.  m = 1 is fr_schedule_find_clear(n_windows, 1, 0,
 * n_windows) job for job. */
int fr_schedule_scan_clear(size_t n_windows, size_t m, int32_t starts, fr_job* jobs, size_t jobs_cap, size_t* n_jobs,
                           uint32_t* level_off, size_t level_cap, size_t* n_levels, int32_t* outs3, size_t outs_cap,
                           size_t* n_outs);
/* fr_plain_find_clear by the scan's route: the windows classed and padded, both lowered programs
 * evaluated over the compacted text, every start given its class's output. */
int fr_plain_scan_clear(const uint8_t* content, size_t len, const uint16_t* masks, size_t m, size_t start_lo,
                        size_t start_hi, uint8_t* starts_out, int32_t* any);
/* The same four for a byte-table needle: a start's (a window's) tests are m terms (table i,
 * position, 0), one extract-sum and one kind-2 job of offset 1 - 2 m per start for m <= 16, else
 * balanced chunks of the m terms and their AND.  tables: 32 bytes per character. */
int fr_schedule_find_clear_bytes(size_t n_chars, size_t m, size_t start_lo, size_t start_hi, int32_t starts,
                                 fr_job* jobs, size_t jobs_cap, size_t* n_jobs, uint32_t* level_off, size_t level_cap,
                                 size_t* n_levels, int32_t* outs3, size_t outs_cap, size_t* n_outs);
int fr_schedule_scan_clear_bytes(size_t n_windows, size_t m, int32_t starts, fr_job* jobs, size_t jobs_cap,
                                 size_t* n_jobs, uint32_t* level_off, size_t level_cap, size_t* n_levels,
                                 int32_t* outs3, size_t outs_cap, size_t* n_outs);
int fr_plain_find_clear_bytes(const uint8_t* content, size_t len, const uint8_t* tables, size_t m, size_t start_lo,
                              size_t start_hi, uint8_t* starts_out, int32_t* any);
int fr_plain_scan_clear_bytes(const uint8_t* content, size_t len, const uint8_t* tables, size_t m, size_t start_lo,
                              size_t start_hi, uint8_t* starts_out, int32_t* any);

/* ----- host-only introspection (tests; no device needed) ----- */
/* Canonical AST string of parse(pattern) (parser.rs:146-185). */
int fr_parse(const char* pattern, char* buf, size_t buflen);
/* Symbolic has_match over a plaintext content string: reference counters and
 * the plaintext result of the recorded circuit and of the lowered PBS program. */
typedef struct {
    uint64_t ct_ops, cache_hits, n_branches;
    uint64_t pbs, levels, max_level_width;
    int32_t result_recorded; /* value of the recorded reference op DAG */
    int32_t result_lowered;  /* value of the lowered PBS program (plaintext LUT semantics) */
} fr_plain_result;
int fr_plain_match(const char* content, size_t len, const char* pattern, size_t start_lo, size_t start_hi,
                   int32_t lowering, fr_plain_result* out);

/* Evaluation engine of the regex (fr_set_engine, fr_plain_match_ex):
 * FR_ENGINE_ENUMERATE: the reference's variant enumeration (engine.rs:45-214),
 *   exact ct_ops / cache_hits; exponential on deep variant trees (BASELINE
 *   config 5 exhausts memory, as in the reference).
 * FR_ENGINE_MERGED: state-merging evaluation (beyond the reference): the same
 *   decrypted result, a circuit polynomial in the content length and of
 *   logarithmic depth for fixed-width loops; ct_ops counts circuit operations.
 * FR_ENGINE_AUTO (default): enumerate within 2^22 variants, else merged. */
enum { FR_ENGINE_AUTO = 0, FR_ENGINE_ENUMERATE = 1, FR_ENGINE_MERGED = 2 };
/* Pattern grammar (fr_set_grammar, fr_parse_ex, fr_plain_match_g):
 * FR_GRAMMAR_REFERENCE (default): parser.rs:146-351 exactly ([a-z0-9] is Err).
 * FR_GRAMMAR_EXT (beyond the reference, opt-in): also bare digits as
 *   characters and bracket classes mixing letters, digits, escapes and
 *   inclusive ranges — [a-z0-9], [^A-Z_], [\-a] — tried only where the
 *   reference grammar fails, so every pattern the reference accepts keeps its
 *   AST (including [a-z]'s strict lower bound, engine.rs:99-111). */
enum { FR_GRAMMAR_REFERENCE = 0, FR_GRAMMAR_EXT = 1 };
int fr_set_grammar(fr_ctx* ctx, int32_t grammar);
int fr_parse_ex(const char* pattern, int32_t grammar, char* buf, size_t buflen);
int fr_plain_match_g(const char* content, size_t len, const char* pattern, size_t start_lo, size_t start_hi,
                     int32_t lowering, int32_t engine, int32_t grammar, fr_plain_result* out);
/* FR_ENGINE_AUTO's decision: the variants the reference's enumeration would build for
 * starts [start_lo, start_hi) of n_chars -- *counted from the AST without building them,
 * *enumerated by running it (enumerate != 0; else 0) -- each saturating at cap + 1.
 * *outcome says whether there is a count: FR_COST_COUNTED; FR_COST_PANIC, where the
 * enumeration would panic (engine.rs:189-190, or a repetition it cannot allocate);
 * FR_COST_MEMORY, where the counter's memo would exceed mem_bytes (0: the bound AUTO uses,
 * 256 MiB; entries and the end positions they store are counted).  Without a count *counted
 * is 0 and AUTO enumerates under its budget, as it would without the counter.  AUTO goes
 * straight to the merged engine iff the count is > 2^22. */
enum { FR_COST_COUNTED = 0, FR_COST_PANIC = 1, FR_COST_MEMORY = 2 };
int fr_debug_enumeration_cost(const char* pattern, int32_t grammar, size_t n_chars, size_t start_lo, size_t start_hi,
                              uint64_t cap, uint64_t mem_bytes, int32_t enumerate, int32_t* outcome,
                              uint64_t* counted, uint64_t* enumerated);
/* fr_plain_match_g of fr_has_match_parts' program: out->result_lowered is the OR of the
 * parts, parts[0..*n_parts) their plaintext values (room for max_parts). */
int fr_plain_match_parts(const char* content, size_t len, const char* pattern, size_t start_lo, size_t start_hi,
                         int32_t lowering, int32_t engine, int32_t grammar, size_t max_parts, fr_plain_result* out,
                         int32_t* parts, size_t* n_parts);
/* ... of fr_match_starts' merged program: lowered[j] / recorded[j] are the plaintext values of
 * start start_lo + j in the lowered program and in that start's recorded circuit, j <
 * *n_starts = start_hi - start_lo <= cap; out's counters are summed over the starts, its
 * results the OR over them, pbs / levels / max_level_width the merged program's. */
int fr_plain_match_starts(const char* content, size_t len, const char* pattern, size_t start_lo, size_t start_hi,
                          int32_t lowering, int32_t engine, int32_t grammar, fr_plain_result* out, int32_t* lowered,
                          int32_t* recorded, size_t cap, size_t* n_starts);
int fr_set_engine(fr_ctx* ctx, int32_t engine);
int fr_plain_match_ex(const char* content, size_t len, const char* pattern, size_t start_lo, size_t start_hi,
                      int32_t lowering, int32_t engine, fr_plain_result* out);

/* lowering modes for fr_plain_match / fr_set_lowering:
 * FR_LOWER_FAITHFUL: one gate group per reference op (eq/gt/le = 3 PBS, and/or = 1,
 *   not linear), in the reference's fold order (engine.rs:22-35: depth #branches).
 * FR_LOWER_THRESHOLD (default): threshold gates of fan-in <= 16, multi-value LUTs.
 * FR_LOWER_FAITHFUL_TREE: FR_LOWER_FAITHFUL's gates, the same PBS count, with every
 *   AND/OR chain whose inner links are used once rebalanced into a binary tree of
 *   least depth (/abc/ x 256: 3,047 PBS in 13 levels, not 257). */
enum { FR_LOWER_FAITHFUL = 0, FR_LOWER_THRESHOLD = 1, FR_LOWER_FAITHFUL_TREE = 2 };
int fr_set_lowering(fr_ctx* ctx, int32_t mode);
/* Multi-value bootstrapping: gates of one level that read the same linear
 * combination share one blind rotation (default on). */
int fr_set_multi_value(fr_ctx* ctx, int32_t on);
/* Device profiling: 0 off; 1 blind-rotation timers (HIP stop events stamped by the
 * launches themselves, hipExtLaunchKernel: no marker packets, no syncs; a level's blind
 * rotation runs from its keyswitch's stop event to its own, the launch gap between them
 * included; what bench.py's timed region uses; FR_TIMER_CHAIN=0 stamps a start event on
 * the blind rotation instead, 9-15 us more per launch); 2 also the keyswitch timers (start
 * and stop events on every level's keyswitch, ~30 us per /abc/ x 256 match).  Timers
 * resolve at the next synchronisation.  Any other value is FR_ERR_INVALID. */
int fr_set_profiling(fr_ctx* ctx, int32_t on);

/* ----- packed results: the host restatement (tests; the device path's reference) ----- */
/* Rows row_lo <= row < row_hi <= 3*kN of the packing key that fr_gen_packing_key_keyed draws
 * under the same key, (row_hi - row_lo)*(k+1)*N words (client key needed).  The whole key
 * takes a few seconds of host time, hence the range. */
int fr_gen_packing_rows_keyed(fr_ctx* ctx, const uint8_t* key /* NULL: OS CSPRNG */, size_t row_lo, size_t row_hi,
                              uint64_t* out);
/* The same rows of the key that fr_gen_packing_key_compact_keyed draws: masks under the mask
 * key, bodies rounded to 40 bits. */
int fr_gen_packing_rows_compact_keyed(fr_ctx* ctx, const uint8_t* key /* NULL: OS CSPRNG */, size_t row_lo,
                                      size_t row_hi, uint64_t* out);
/* fr_pack_bools in plain host loops, on LWEs given as words: boolean j is
 * off[j]*2^58 + w[j]*lwes[j] (w, off NULL: 1, 0; w[j] == 0: a constant, lwes[j] is not read,
 * and lwes may be NULL if every w[j] is 0).  Needs the packing key; on a device context the
 * rows are downloaded for the call. */
int fr_pack_lwes(fr_ctx* ctx, const uint64_t* lwes /* n*(kN+1) */, const int32_t* w, const int32_t* off, size_t n,
                 uint64_t* out_words /* (k+1)*N */);
/* phase[t] = coefficient t of B - sum_c A_c*S_c (negacyclic) of a packed result's words under
 * the client key: N words. */
int fr_packed_phase(fr_ctx* ctx, const uint64_t* words, uint64_t* phase);

/* ----- single-stage device entry points (parity tests of each kernel) ----- */
/* in: count*(kN+1) torus LWEs -> out: count*(n+1) keyswitched LWEs */
int fr_dev_keyswitch(fr_ctx* ctx, const uint64_t* in, size_t count, uint64_t* out);
/* Column col < (k+1)*N of the packing key's byte-limb operand (what the packing GEMM reads),
 * its 8 limbs recombined on the device: out[r] must be word col of row r, r < 3*kN. */
int fr_dev_packing_limb_column(fr_ctx* ctx, int32_t col, uint64_t* out /* 3*kN */);
/* in: count*(n+1) keyswitched LWEs, luts: count*16 -> out: count*(kN+1) */
int fr_dev_blind_rotate(fr_ctx* ctx, const uint64_t* in, const uint8_t* luts, size_t count, uint64_t* out);
/* one blind rotation with n_out LUTs (direct: n_out == 1, LUT polynomial
 * rotated itself; else multi-value) -> out: n_out*(kN+1) */
int fr_dev_blind_rotate_multi(fr_ctx* ctx, const uint64_t* in, const uint8_t* luts, int32_t n_out, int32_t direct,
                              uint64_t* out);
/* one launch of `count` selector jobs (private search; FFT ring): rotation i starts from the
 * GLWE ciphertext accs + i*(k+1)*N instead of a LUT's test polynomial -> out: count*(kN+1).  A
 * trivial selector (zero masks, body the direct test polynomial of a LUT) gives
 * fr_dev_blind_rotate's words.  The launch shape follows count, as every launch's does. */
int fr_dev_blind_rotate_acc(fr_ctx* ctx, const uint64_t* in /* count*(n+1) */, const uint64_t* accs, size_t count,
                            uint64_t* out);
/* the extract-sum kernel alone (private search over clear content; FFT ring): sum i < n_sums has
 * n_terms[i] terms, each 3 words (selector q, content position pos, half h) following those of
 * sum i - 1 in `terms`, and is the sum over them of the sample extract of the needle's selector q
 * at coefficient ((content[pos] >> 4 h) & 15) N/16 -> out: n_sums*(kN+1), wrapping u64, exact.
 * FR_ERR_INVALID for n_terms outside [1, 16], q >= 2 m, pos >= len, h > 1, before any launch.
 * With a byte-table needle a term is (table i, pos, 0): the extract of selector i / (N/256) at
 * coefficient (i % (N/256)) 256 + content[pos]; i >= m or a non-zero third word is refused.
 * fr_dev_select_sum_ms: the kernel's HIP-event ms of the last call under fr_set_profiling. */
int fr_dev_select_sum(fr_ctx* ctx, const fr_needle* needle, const uint8_t* content, size_t len,
                      const int32_t* terms /* 3 per term */, const int32_t* n_terms, size_t n_sums, uint64_t* out);
int fr_dev_select_sum_ms(fr_ctx* ctx, double* ms);
/* The mapped pack alone (a scan's reply): n_rows boolean handles, and n starts of which start j
 * is the boolean bools[map[j]] or, where map[j] < 0, the constant 0; buf receives the FRPKRES1
 * (compact = 0) or FRCPRES1 blob of the n starts (buf NULL: size query).  The identity map gives
 * fr_pack_bools_blob's bytes.  FR_ERR_INVALID before anything is staged for n_rows < 1,
 * n_rows > n, n > N, an entry >= n_rows and a row no start reads.  fr_device_timers_pack holds its
 * stages.  fr_pack_lwes_mapped is the host restatement (plain loops, exact mod 2^64) in
 * fr_pack_lwes' terms: lwes, w, off have n_rows entries. */
int fr_dev_pack_mapped(fr_ctx* ctx, const fr_ct* bools, size_t n_rows, const int32_t* map, size_t n, int32_t compact,
                       uint8_t* buf, size_t cap, size_t* written);
int fr_pack_lwes_mapped(fr_ctx* ctx, const uint64_t* lwes, const int32_t* w, const int32_t* off, size_t n_rows,
                        const int32_t* map, size_t n, uint64_t* out_words);
/* negacyclic product in Z_Q[X]/(X^N+1) (Q = 998244353 * 1004535809, inputs in
 * [0, Q)) through the device RNS NTT: count pairs */
int fr_dev_ring_mul(fr_ctx* ctx, const uint64_t* a, const uint64_t* b, size_t count, uint64_t* out);
/* Full timed PBS batch for roofline measurement: count gates of the given
 * lut over the uploaded boolean/radix handles; returns BR kernel ms. */
int fr_dev_bench_pbs(fr_ctx* ctx, const fr_ct* in, size_t count, int32_t iters, double* br_ms, double* total_ms);

int fr_device_info(fr_ctx* ctx, char* buf, size_t buflen);

/* Scalar maps shared by host and device code (test hook): op 0 = CRT of the
 * residues of x (identity on [0, Q)), 1 = PBS gadget digit of x mod Q (signed,
 * as u64), 2 = Z_Q -> 2^64 torus of x mod Q (from its residues),
 * 3 = modulus switch of x to 2^y, 4 = keyswitch digit y (0..4) of x (signed, as u64),
 * 5 = the step-schedule entry x with its field y >> 12 (0..4) set to y & 0xFFF,
 * 6 = field y (0..4) of the step-schedule entry x. */
uint64_t fr_debug_scalar(int32_t op, uint64_t x, uint64_t y);
/* The slot arena (test hook): synchronises every lane, so that slots whose release was
 * deferred are recycled, then *slots = the slots ever handed out (the high-water mark) and
 * *free_slots = the length of the free list; slots - free_slots are held by handles, cached
 * plans and shard plans. */
int fr_debug_arena_stats(fr_ctx* ctx, uint64_t* slots, uint64_t* free_slots);
/* The handle table (test hook): *live = the handles not yet released. */
int fr_debug_handle_count(fr_ctx* ctx, uint64_t* live);

#ifdef __cplusplus
}
#endif
#endif
