// Client key (reference fixture layout), deterministic server-key generation,
// client-side encryption — host C++.  The wire blobs that carry them are wire.h's.
#pragma once
#include <cstdint>
#include <vector>

#include "chacha.h"
#include "common.h"

namespace fr {

// ChaCha20 (DJB layout: 64-bit block counter, 64-bit stream id) under a 256-bit
// RngKey (chacha.h): RngKey::from_seed for the reproducible draws of tests,
// benchmarks and multi-rank keygen, from_bytes for a caller's key, from_os for the
// OS CSPRNG.  u64 number idx of a stream is words 2*(idx%8), 2*(idx%8)+1 of
// block idx/8 — random access, so keygen is parallel and deterministic.
enum Stream : uint64_t {
    STREAM_KSK_MASK = 1,
    STREAM_KSK_NOISE = 2,
    STREAM_BSK_MASK = 3,
    STREAM_BSK_NOISE = 4,
    STREAM_ENC_MASK = 5,
    STREAM_ENC_NOISE = 6,
    STREAM_CLIENT_KEY = 7,
    STREAM_MASK_KEY = 8,  // block 0, words 0..7: the public mask key of a compact server key or content blob
    STREAM_PKSK_MASK = 9,
    STREAM_PKSK_NOISE = 10,
    STREAM_NEEDLE_MASK = 11,
    STREAM_NEEDLE_NOISE = 12,
    STREAM_NEEDLE_BYTES_MASK = 13,
    STREAM_NEEDLE_BYTES_NOISE = 14,
};

class Rng {
  public:
    Rng(const RngKey& key, uint64_t stream) : key_(key), stream_(stream) {}
    ~Rng();  // wipes its copy of the key and the last block
    Rng(const Rng&) = delete;
    Rng& operator=(const Rng&) = delete;
    uint64_t u64(uint64_t idx);
    // Box-Muller on words 2*idx, 2*idx+1; z * sigma * scale rounded to an
    // integer (scale 2^64: torus units; scale Q: units of Z_Q).
    int64_t gaussian(uint64_t idx, double sigma, double scale = 18446744073709551616.0);

  private:
    RngKey key_;
    uint64_t stream_, blk_ = 0;
    bool valid_ = false;
    uint32_t w_[16];
};

struct ClientKey {
    std::vector<uint64_t> s_big;    // flattened GLWE key (2048 bits)
    std::vector<uint64_t> s_small;  // LWE key after keyswitch (742 bits)
    int n = 0, k = 0, N = 0;
    int pbs_base_log = 0, pbs_level = 0, ks_base_log = 0, ks_level = 0;
    double lwe_sigma = 0, glwe_sigma = 0;
    uint64_t message_modulus = 0, carry_modulus = 0, num_blocks = 0;
    // the remaining words of the bincode layout, kept as read so that
    // serialize_client_key(parse_client_key(b)) == b: the GLWE key's own data
    // (equal to s_big in every tfhe-rs key) and polynomial_size, and the 17 words
    // of the parameter block + num_blocks (offsets 38736..38871)
    std::vector<uint64_t> s_glwe;
    uint64_t glwe_poly_size = 0;
    uint64_t raw_params[17] = {};
};

// Parse the bincode RadixClientKey of the reference fixture.
ClientKey parse_client_key(const uint8_t* data, size_t len);
// The same layout written back (engine.rs:238-246 generate_test_keys: bincode::serialize
// of the RadixClientKey); byte-identical to the blob a key was parsed from.
std::vector<uint8_t> serialize_client_key(const ClientKey& ck);
// A fresh RadixClientKey (gen_keys_radix(&PARAM_MESSAGE_2_CARRY_2, 4), ciphertext.rs:42-45):
// uniform binary GLWE key of k*N bits (its flattening is the big LWE key) and uniform binary
// LWE key of n bits, from the ChaCha20 stream STREAM_CLIENT_KEY of `key`; parameter block
// from p (PARAM_MESSAGE_2_CARRY_2's words at the default params: pfks = (1, 2^23, glwe
// sigma), cbs = (0, 0), message and carry modulus 4, 4 blocks).
ClientKey gen_client_key(const Params& p, const RngKey& key);

// KSK: [i in kN][level j][t in n+1], torus 2^64.
void gen_ksk(const Params& p, const ClientKey& ck, const RngKey& key, std::vector<uint64_t>& ksk);
// the same rows with the masks drawn under mask_key and the noise under noise_key
void gen_ksk(const Params& p, const ClientKey& ck, const RngKey& mask_key, const RngKey& noise_key,
             std::vector<uint64_t>& ksk);
// BSK: [GGSW w][row r in k+1][component c in k+1][coef], coefficient domain mod Q (rns.h);
// GGSW w per Params::bsk_unroll (k = 1: 3 per pair of LWE coefficients).
void gen_bsk(const Params& p, const ClientKey& ck, const RngKey& key, std::vector<uint64_t>& bsk);
// Host parts of the device key generator (Device::gen_server_key): the
// Box-Muller noise of every KSK row (lwe sigma, torus units), of every BSK
// body coefficient ([w][r][coef], glwe sigma, torus units) and the message bit
// of every GGSW.
void gen_ksk_noise(const Params& p, const RngKey& key, std::vector<int64_t>& e);
void gen_bsk_noise_torus(const Params& p, const RngKey& key, std::vector<int32_t>& e);
std::vector<uint8_t> ggsw_messages(const Params& p, const ClientKey& ck);

// Compact (seeded) server key, FFT ring.  Every mask word is a ChaCha20
// word of a public mask key, words 0..7 of chacha_block(K, STREAM_MASK_KEY, 0) for the
// call's secret generator key K, at the index the standard generator uses; the noise is
// the standard generator's under K.  No secret touches a mask: the gadget term m_w g
// that the standard form adds to coefficient 0 of mask polynomial r (rows r < k) sits in
// the body as -m_w g S_r, so the phase B - sum_j A_j S_j of every row is the standard
// form's polynomial.  The key is then its bodies and the 32 bytes of the mask key.
RngKey derive_mask_key(const RngKey& key);
// the full arrays (gen_ksk's and gen_bsk's layouts) and the mask key
void gen_server_key_compact(const Params& p, const ClientKey& ck, const RngKey& key, std::vector<uint64_t>& ksk,
                            std::vector<uint64_t>& bsk, RngKey& mask_key);
// the body counts of its wire blob (wire.h), u64 each
size_t compact_ksk_bodies(const Params& p);
size_t compact_bsk_bodies(const Params& p);

// Packing key (DESIGN.md §1 "Packed results"): row 3 i + l, i < kN, l < PK_LEVELS, is a GLWE
// encryption under the GLWE key (the big key read as k polynomials) of the constant polynomial
// s_big[i] 2^(64 - PK_BASE_LOG (l + 1)): k mask polynomials, then the body, (k+1) N words.
// Mask polynomial j of a row is u64 numbers (row k + j) N + t of STREAM_PKSK_MASK, the body's
// noise numbers row N + t of STREAM_PKSK_NOISE (the BSK generator's indexing).
inline size_t pk_rows(const Params& p) { return (size_t)p.big() * PK_LEVELS; }
inline size_t pk_row_words(const Params& p) { return (size_t)(p.k + 1) * p.N; }
inline size_t pk_len(const Params& p) { return pk_rows(p) * pk_row_words(p); }
// rows row_lo <= row < row_hi into out[(row_hi - row_lo) * pk_row_words]; the whole key takes
// a few seconds of host time (each row is k N^2 / 2 additions), hence the range
void gen_packing_rows(const Params& p, const ClientKey& ck, const RngKey& key, size_t row_lo, size_t row_hi,
                      uint64_t* out);
// the same rows with the masks drawn under mask_key and the noise under noise_key; round40:
// every body word rounded to its top PKC_BODY_BITS bits (the compact form below)
void gen_packing_rows(const Params& p, const ClientKey& ck, const RngKey& mask_key, const RngKey& noise_key,
                      bool round40, size_t row_lo, size_t row_hi, uint64_t* out);
// the body noise of every row for the device generator ([row][N], glwe sigma, torus units)
void gen_pksk_noise(const Params& p, const RngKey& key, std::vector<int32_t>& e);

// Compact (seeded) packing key, every ring.  The masks are ChaCha20 words of
// the public mask key M = derive_mask_key(K) at the standard generator's indices, the noise is
// the standard generator's under the call's secret key K, and the message sits on the body's
// coefficient 0, so no mask word carries a secret.  The body B travels rounded to 40 bits,
// b40 = ((B + 2^23) >> 24) mod 2^40, and is installed as b40 << 24 on both sides: installed - B
// lies in (-2^23, 2^23] (a 2^-16 share of the gadget's own rounding variance).
// The installed key is an ordinary packing key.
constexpr int PKC_BODY_BITS = 40, PKC_DROP_BITS = 64 - PKC_BODY_BITS;
inline uint64_t pk_round40(uint64_t body) { return (body + ((uint64_t)1 << (PKC_DROP_BITS - 1))) >> PKC_DROP_BITS; }
// The blob (wire.h) carries b40 in a u32 plane (b40 >> 8) and a u8 plane (b40 & 0xFF).
inline size_t pk_compact_planes(const Params& p) { return 5 * pk_rows(p) * (size_t)p.N; }  // bytes

// Packing keyswitch, host restatement (plain loops; the device path is keyswitch.hip's):
//   out = sum_j X^j ((0, .., 0, b_j) - sum_{i,l} d_{j,i,l} PKSK[3 i + l])
// over (Z_2^64[X] / (X^N + 1))^(k+1), for the n <= N booleans c_j = off_j 2^58 + w_j lwe_j
// (w, off NULL: 1, 0; w_j = 0: a constant, its LWE is not read), d the signed base-2^7
// digits of the mask of c_j rounded to 21 bits.  Exact mod 2^64.
void pack_host(const Params& p, const uint64_t* pksk, const uint64_t* lwes, const int32_t* w, const int32_t* off,
               size_t n, uint64_t* out /* (k+1) N */);
// The same pack where several starts share a row (a scan's window classes, fr_scan_clear_starts):
//   out = sum_{j < n, map[j] >= 0} X^j G[map[j]]
// with G[r] the keyswitched row of boolean r < R as above (lwes, w, off have R entries).  By
// linearity this is pack_host over the rows expanded start by start, a start with map[j] < 0 the
// constant 0.  check_pack_map refuses R < 1, R > n, n > N, an entry >= R and a row no start reads.
void check_pack_map(const int32_t* map, size_t n, size_t R, size_t N);
void pack_host_mapped(const Params& p, const uint64_t* pksk, const uint64_t* lwes, const int32_t* w,
                      const int32_t* off, size_t R, const int32_t* map, size_t n, uint64_t* out /* (k+1) N */);
// Compact packed result.  A packed boolean is never bootstrapped again, so
// only the client's rounding at Delta / 2 = 2^58 sees its error: every coefficient travels
// rounded to its top 16 bits, v = ((x + 2^47) >> 48) mod 2^16, and is installed as v << 48, the
// mask and the body alike; the body coefficients past n carry no boolean and are not sent.
// The rounding adds std sqrt((h + 1) / 12) 2^48 to the phase, h the key's weight: 2^51.2 at
// h = 1024 against the 2^58 threshold.
// Decryption is glwe_phase of the expanded words and round(phase / 2^59) & 1 for j < n.
constexpr int PKCRES_BITS = 16, PKCRES_DROP = 64 - PKCRES_BITS;
inline uint16_t packed_round16(uint64_t x) { return (uint16_t)((x + ((uint64_t)1 << (PKCRES_DROP - 1))) >> PKCRES_DROP); }
inline size_t packed_compact_values(const Params& p, size_t n) { return (size_t)p.big() + n; }  // u16 values
// phase B - sum_c A_c S_c (negacyclic) of a GLWE ciphertext under the client key: N words
void glwe_phase(const Params& p, const ClientKey& ck, const uint64_t* ct, uint64_t* phase);

// noise of encrypt_blocks for blocks first_block .. first_block + count - 1
void enc_noise(const Params& p, const RngKey& key, uint64_t first_block, size_t count, std::vector<int64_t>& e);

// Fresh LWE encryptions of block messages (Delta = 2^59) under the big key.
void encrypt_blocks(const Params& p, const ClientKey& ck, const uint8_t* msgs, size_t count, const RngKey& key,
                    uint64_t first_block, uint64_t* out /* count * (kN+1) */);
// the same blocks with the masks drawn under mask_key and the noise under noise_key
void encrypt_blocks(const Params& p, const ClientKey& ck, const uint8_t* msgs, size_t count, const RngKey& mask_key,
                    const RngKey& noise_key, uint64_t first_block, uint64_t* out /* count * (kN+1) */);

// Compact (seeded) content ciphertexts, both rings.  The masks of the blocks
// are ChaCha20 words of the public mask key derive_mask_key(K) at the standard encryptor's
// indices (u64 number (first_block + q) kN + t of STREAM_ENC_MASK); the noise is the standard
// encryptor's under the call's secret key K.  An LWE mask is public anyway, so no secret
// touches a mask word, and the ciphertexts are their bodies and the 32 bytes of the mask key.
// encrypt_blocks under (derive_mask_key(key), key) as the content blob of wire.h; `key` is the
// caller's to wipe
std::vector<uint8_t> encrypt_content_blob(const Params& p, const ClientKey& ck, const uint8_t* msgs, size_t count,
                                          const RngKey& key, uint64_t first_block);
// Private search: an encrypted needle, FFT ring.  A selector is a GLWE
// ciphertext, k mask polynomials then the body, (k+1) N words, under the GLWE key (the big key
// read as k polynomials) whose phase is the direct test polynomial V(T) of a 0/1 table T of
// the 16 nibble values: boxes of N/16 recentred by half a box, -T[0] in the last half box,
// T[s] 2^59 (needle_test_poly: the device's test_poly).  A needle of m characters is 2 m
// selectors, selector 2 i + h the table of nibble h (0: low) of character i, a table the
// 16-bit mask of its accepted values.  Mask word t of mask polynomial c of selector q is u64
// number (q k + c) N + t of STREAM_NEEDLE_MASK under the public mask key M = derive_mask_key(K);
// the noise is the gaussian (glwe sigma) of STREAM_NEEDLE_NOISE under the call's secret key K
// at q N + t; body = sum_c A_c S_c + V(T_q) + e, negacyclic.  No secret touches a mask word.
inline size_t needle_words(const Params& p, size_t m) { return 2 * m * (size_t)(p.k + 1) * p.N; }
uint64_t needle_test_poly(int N, int t, uint16_t table);
// the needle blob of wire.h; masks: lo, hi per character (2 m tables); `key` is the caller's to wipe
std::vector<uint8_t> encrypt_needle_blob(const Params& p, const ClientKey& ck, const uint16_t* masks, size_t m,
                                         const RngKey& key);
// A byte-table needle (private search over clear content only): character i is one 0/1 table T_i
// of the 256 byte values, 32 bytes, bit b at tables[32 i + b / 8] >> (b % 8).  N / 256 tables
// share a selector: the phase of coefficient (i % (N/256)) 256 + b of selector i / (N/256) is
// T_i[b] 2^59 -- no boxes, no recentring, no sign, because the server sample-extracts exactly that
// coefficient; the coefficients past the last table encrypt 0.  Masks and noise as the nibble
// needle's, on STREAM_NEEDLE_BYTES_MASK under M and STREAM_NEEDLE_BYTES_NOISE under K.
inline size_t needle_bytes_per_selector(const Params& p) { return (size_t)p.N / 256; }
inline size_t needle_bytes_selectors(const Params& p, size_t m) {
    return (m + needle_bytes_per_selector(p) - 1) / needle_bytes_per_selector(p);
}
inline size_t needle_bytes_words(const Params& p, size_t m) {
    return needle_bytes_selectors(p, m) * (size_t)(p.k + 1) * p.N;
}
// the byte-table needle blob of wire.h; `key` is the caller's to wipe
std::vector<uint8_t> encrypt_needle_bytes_blob(const Params& p, const ClientKey& ck, const uint8_t* tables, size_t m,
                                               const RngKey& key);
uint64_t lwe_phase(const Params& p, const ClientKey& ck, const uint64_t* lwe);
// tfhe-rs shortint decrypt_message_and_carry: round(phase / Delta) mod 16
uint32_t decode16(uint64_t phase);

// Host negacyclic NTT over Z_p for the two RNS primes (merged-psi
// Cooley-Tukey / Gentleman-Sande, bit-reversed evaluation order) — used by
// keygen and for the device twiddles.  Canonical residues, plain '%' math.
struct NttTables {
    int N = 0, logN = 0;
    std::vector<uint32_t> zeta[2], izeta[2];  // zeta[k] = psi^brv(k), izeta[k] = psi^-brv(k)
    uint32_t n_inv[2] = {0, 0};
    explicit NttTables(int N);
    void forward(int q, uint32_t* a) const;
    void inverse(int q, uint32_t* a) const;  // includes the 1/N factor
};
// negacyclic product mod Q of a, b in [0, Q)
void ring_mul_q(const NttTables& T, const uint64_t* a, const uint64_t* b, uint64_t* out);

}  // namespace fr
