// The eight wire blobs (include/fheregex.h states each format): header sizes, blob sizes,
// writers, checkers and the expansions that need no secret; little endian.  What the blobs carry
// -- keys, ciphertexts, their randomness and rounding -- is keys.h's.  Every check_* throws
// Error(FR_ERR_INVALID) unless the whole header and the exact length are the context's; it
// allocates nothing, so a caller runs it before it touches an installed key.  A payload starts at
// blob + X_HEADER; wire.cpp states each header's layout once, for its writer and its checker
// alike, and asserts X_HEADER against it at compile time.
#pragma once
#include <cstdint>
#include <vector>

#include "keys.h"

namespace fr {

void put_le32(uint8_t* o, uint32_t v);
void put_le64(uint8_t* o, uint64_t v);
uint32_t get_le32(const uint8_t* o);
uint64_t get_le64(const uint8_t* o);

// ---- "FRCSKEY1", the compact server key (FFT ring): eight int32 parameters, the mask key, the
// KSK bodies [kN * ks_level], the BSK bodies [W][k+1][N]
constexpr size_t COMPACT_HEADER = 72;
size_t compact_size(const Params& p);  // bytes
RngKey check_compact(const Params& p, const uint8_t* blob, size_t len);  // the mask key
void pack_compact(const Params& p, const RngKey& mask_key, const std::vector<uint64_t>& ksk,
                  const std::vector<uint64_t>& bsk, uint8_t* out /* compact_size bytes */);
// check_compact, then every mask from the mask key (returned) around the blob's bodies
RngKey expand_compact(const Params& p, const uint8_t* blob, size_t len, std::vector<uint64_t>& ksk,
                      std::vector<uint64_t>& bsk);

// ---- "FRPKKEY1", the packing key: the eight int32 parameters, PK_BASE_LOG, PK_LEVELS, the rows
constexpr size_t PK_HEADER = 48;
inline size_t pk_blob_size(const Params& p) { return PK_HEADER + 8 * pk_len(p); }
void write_pk_header(const Params& p, uint8_t* out /* PK_HEADER bytes */);
void check_pk_blob(const Params& p, const uint8_t* blob, size_t len);

// ---- "FRCPKEY1", the compact packing key: the eight int32 parameters, the gadget, the body
// bits, a reserved zero, the mask key, 8 zero bytes, then the high plane u32[3kN][N] (b40 >> 8)
// and the low plane u8[3kN][N] (b40 & 0xFF)
constexpr size_t PKC_HEADER = 96;
inline size_t pk_compact_size(const Params& p) { return PKC_HEADER + pk_compact_planes(p); }
void write_pk_compact_header(const Params& p, const RngKey& mask_key, uint8_t* out /* PKC_HEADER bytes */);
RngKey check_pk_compact(const Params& p, const uint8_t* blob, size_t len);  // the mask key
// the bodies of full rows [pk_rows][(k+1) N] into the two planes (pk_compact_planes bytes)
void pack_pk_compact(const Params& p, const uint64_t* rows, uint8_t* planes);
// check_pk_compact, then the full rows: every mask from the mask key (returned), every body b40 << 24
RngKey expand_pk_compact(const Params& p, const uint8_t* blob, size_t len, std::vector<uint64_t>& rows);

// ---- "FRPKRES1", the packed result: int32 k, N, u64 n (1 <= n <= N), then the (k+1) N words
constexpr size_t PKRES_HEADER = 24;
inline size_t packed_result_size(const Params& p) { return PKRES_HEADER + 8 * pk_row_words(p); }
void write_packed_result(const Params& p, size_t n, const uint64_t* words, uint8_t* out);
size_t check_packed_result(const Params& p, const uint8_t* blob, size_t len);  // n

// ---- "FRCPRES1", the compact packed result: int32 k, N, u64 n, u32 16 (coefficient bits), u32 0
// (reserved), then u16 mask[kN], u16 body[n]; exactly 32 + 2 (kN + n) bytes.  The coefficients
// past n were not sent (they expand to a zero body), so there is nothing to check there, unlike
// check_packed_result's blob.
constexpr size_t PKCRES_HEADER = 32;
inline size_t packed_compact_size(const Params& p, size_t n) { return PKCRES_HEADER + 2 * packed_compact_values(p, n); }
// the blob of the packed_compact_values(p, n) rounded values (packed_round16) of a packed GLWE
void write_packed_compact(const Params& p, size_t n, const uint16_t* values, uint8_t* out);
// the blob of a packed GLWE's (k+1) N words carrying n booleans: plain loops, the word-for-word
// reference of the device's k_pack_compress
void compress_packed(const Params& p, size_t n, const uint64_t* words, uint8_t* out);
size_t check_packed_compact(const Params& p, const uint8_t* blob, size_t len);  // n
// check_packed_compact, then the blob's (k+1) N words: v << 48, the body past n zero; n
size_t expand_packed_compact(const Params& p, const uint8_t* blob, size_t len, uint64_t* words);

// ---- "FRCCTXT1", compact content: int32 k, N, u64 first_block, u64 n_blocks, the mask key,
// n_blocks u64 bodies; exactly 64 + 8 n_blocks bytes
constexpr size_t CONTENT_HEADER = 64;
constexpr uint64_t CONTENT_MAX_BLOCK = (uint64_t)1 << 40;  // first_block + n_blocks: (f + q) kN / 8 cannot wrap
struct ContentBlob {
    RngKey mask_key;
    uint64_t first_block = 0;
    size_t n_blocks = 0;
    const uint8_t* bodies = nullptr;  // n_blocks u64, little endian, any alignment
};
size_t content_blob_size(size_t n_blocks);  // bytes; Error(FR_ERR_INVALID) past CONTENT_MAX_BLOCK blocks
// Error(FR_ERR_INVALID) unless first_block + n_blocks <= CONTENT_MAX_BLOCK, each term tested before the sum
void check_content_range(uint64_t first_block, uint64_t n_blocks);
void write_content_header(const Params& p, uint64_t first_block, size_t n_blocks, const RngKey& mask_key,
                          uint8_t* out /* CONTENT_HEADER bytes */);
// also refused: first_block + n_blocks > 2^40 and (radix: the string entries) n_blocks % 4 != 0
ContentBlob check_content_blob(const Params& p, const uint8_t* blob, size_t len, bool radix);
// check_content_blob (radix = false), then every mask from the mask key around the blob's
// bodies; out has n_blocks * (kN+1) words.  Needs no client key.
void expand_content(const Params& p, const uint8_t* blob, size_t len, uint64_t* out);

// ---- "FRNEEDL1", the needle (FFT ring): int32 k, N, u64 m (1 <= m <= 64), the mask key, 8 zero
// bytes, then the 2 m body polynomials of N u64; exactly 64 + 16 m N bytes
constexpr size_t NEEDLE_HEADER = 64;
size_t needle_blob_size(const Params& p, size_t m);  // Error(FR_ERR_INVALID) unless 1 <= m <= 64
struct NeedleBlob {
    RngKey mask_key;
    size_t m = 0;
    const uint8_t* bodies = nullptr;  // 2 m N u64, little endian, any alignment
};
void write_needle_header(const Params& p, size_t m, const RngKey& mask_key, uint8_t* out /* NEEDLE_HEADER bytes */);
NeedleBlob check_needle_blob(const Params& p, const uint8_t* blob, size_t len);
// check_needle_blob, then every mask from the mask key around the blob's bodies: out has
// needle_words(p, m) words, [selector][polynomial][N].  Needs no client key.
void expand_needle(const Params& p, const uint8_t* blob, size_t len, uint64_t* out);

// ---- "FRNEEDB1", the byte-table needle (FFT ring, clear content only): FRNEEDL1's header under
// its own magic, then the G = ceil(256 m / N) body polynomials of N u64 (N / 256 tables of 256
// coefficients each per polynomial); exactly 64 + 8 G N bytes
size_t needle_bytes_blob_size(const Params& p, size_t m);  // Error(FR_ERR_INVALID) unless 1 <= m <= 64
// true: the blob begins with this format's magic (fr_upload_needle tells the two needles apart)
bool is_needle_bytes_blob(const uint8_t* blob, size_t len);
void write_needle_bytes_header(const Params& p, size_t m, const RngKey& mask_key, uint8_t* out /* NEEDLE_HEADER bytes */);
NeedleBlob check_needle_bytes_blob(const Params& p, const uint8_t* blob, size_t len);  // bodies: G N u64
// check_needle_bytes_blob, then every mask from the mask key around the blob's bodies: out has
// needle_bytes_words(p, m) words, [selector][polynomial][N].  Needs no client key.
void expand_needle_bytes(const Params& p, const uint8_t* blob, size_t len, uint64_t* out);

}  // namespace fr
