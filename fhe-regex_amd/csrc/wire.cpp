// The wire blobs' framing (wire.h).  Each format's header is one function, *_layout, over a
// cursor that stores the header, checks one -- the refusals in the order they are stated -- or
// counts its bytes at compile time.  No byte offset of a header is written anywhere else.
#include "wire.h"

#include <cstring>

#include "parallel.h"

namespace fr {

void put_le64(uint8_t* o, uint64_t v) {
    for (int i = 0; i < 8; ++i) o[i] = (uint8_t)(v >> (8 * i));
}
void put_le32(uint8_t* o, uint32_t v) {
    for (int i = 0; i < 4; ++i) o[i] = (uint8_t)(v >> (8 * i));
}
uint64_t get_le64(const uint8_t* o) { return get_le32(o) | ((uint64_t)get_le32(o + 4) << 32); }
uint32_t get_le32(const uint8_t* o) {
    return (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16) | ((uint32_t)o[3] << 24);
}

namespace {

[[noreturn]] void refuse(const char* why) { throw Error(FR_ERR_INVALID, why); }
void need(bool ok, const char* why) {
    if (!ok) refuse(why);
}

// ---------------------------------------------------------------- the cursor
// A header's fields: an 8-byte magic, a u32 of a fixed value, a u64 the blob carries, the 32-byte
// mask key, zero padding, and `need`, a condition on what was read so far (a count's range, the
// exact length) that sits where its refusal is due.  With `out` the cursor stores them, with `in`
// it checks them, each refusal with its own text, and with neither it counts the bytes.
struct Cursor {
    const uint8_t* in = nullptr;
    uint8_t* out = nullptr;
    size_t n = 0;
    constexpr void magic(const char* m, const char* why) {
        if (out) std::memcpy(out + n, m, 8);
        else if (in && std::memcmp(in + n, m, 8)) refuse(why);
        n += 8;
    }
    constexpr void u32(uint32_t v, const char* why) {
        if (out) put_le32(out + n, v);
        else if (in && get_le32(in + n) != v) refuse(why);
        n += 4;
    }
    constexpr void u64(uint64_t& v) {
        if (out) put_le64(out + n, v);
        else if (in) v = get_le64(in + n);
        n += 8;
    }
    constexpr void key(RngKey& k) {
        for (int i = 0; out && i < 8; ++i) put_le32(out + n + 4 * i, k.w[i]);
        if (in) k = RngKey::from_bytes(in + n);
        n += 32;
    }
    constexpr void zeros(size_t z, const char* why) {
        for (size_t i = 0; i < z; ++i)
            if (out) out[n + i] = 0;
            else if (in && in[n + i]) refuse(why);
        n += z;
    }
    template <class F>
    constexpr void need(F&& ok, const char* why) {
        if (in && !ok()) refuse(why);
    }
    // the eight int32 parameters of the three key blobs; (k, N); the packing gadget
    constexpr void params(const Params& p, const char* why) {
        for (int v : {p.k, p.N, p.n, p.ks_base_log, p.ks_level, p.pbs_base_log, p.pbs_level, p.ring})
            u32((uint32_t)v, why);
    }
    constexpr void k_N(const Params& p, const char* why) { u32((uint32_t)p.k, why), u32((uint32_t)p.N, why); }
    constexpr void gadget(const char* why) { u32((uint32_t)PK_BASE_LOG, why), u32((uint32_t)PK_LEVELS, why); }
};

// what a header carries beside the context's parameters, and what its checks depend on
struct Fields {
    uint64_t count = 0, first_block = 0;  // n, n_blocks or m
    RngKey mask_key{};
    size_t len = 0;      // the blob's length: two formats' lengths depend on their count
    bool radix = false;  // content: a string, whole characters only
};

// ---------------------------------------------------------------- the eight layouts
constexpr void compact_layout(Cursor& c, const Params& p, Fields& f) {
    c.magic("FRCSKEY1", "compact server key: bad magic");
    c.params(p, "compact server key: parameters do not match the context params");
    c.key(f.mask_key);
}

constexpr void pk_layout(Cursor& c, const Params& p, Fields&) {
    c.magic("FRPKKEY1", "packing key: bad magic");
    c.params(p, "packing key: parameters do not match the context params");
    c.gadget("packing key: gadget other than base 2^7, 3 levels");
}

constexpr void pk_compact_layout(Cursor& c, const Params& p, Fields& f) {
    c.magic("FRCPKEY1", "compact packing key: bad magic");
    c.params(p, "compact packing key: parameters do not match the context params");
    c.gadget("compact packing key: gadget other than base 2^7, 3 levels");
    c.u32((uint32_t)PKC_BODY_BITS, "compact packing key: body bits other than 40");
    c.u32(0, "compact packing key: reserved word is not zero");
    c.key(f.mask_key);
    c.zeros(8, "compact packing key: pad bytes are not zero");
}

constexpr void packed_result_layout(Cursor& c, const Params& p, Fields& f) {
    c.magic("FRPKRES1", "packed result: bad magic");
    c.k_N(p, "packed result: k, N do not match the context params");
    c.u64(f.count);
    c.need([&] { return f.count >= 1 && f.count <= (uint64_t)p.N; }, "packed result: n outside 1..N");
}

const char PKCRES_LENGTH[] = "compact packed result: length is not 32 + 2 (kN + n) (fr_packed_compact_size)";
constexpr void packed_compact_layout(Cursor& c, const Params& p, Fields& f) {
    c.magic("FRCPRES1", "compact packed result: bad magic");
    c.k_N(p, "compact packed result: k, N do not match the context params");
    c.u64(f.count);
    c.need([&] { return f.count >= 1 && f.count <= (uint64_t)p.N; }, "compact packed result: n outside 1..N");
    c.u32((uint32_t)PKCRES_BITS, "compact packed result: coefficient bits other than 16");
    c.u32(0, "compact packed result: reserved word not zero");
    c.need([&] { return f.len == packed_compact_size(p, (size_t)f.count); }, PKCRES_LENGTH);
}

const char CONTENT_RANGE[] = "compact content: first_block + n_blocks exceeds 2^40";
// (each term first: the sum of two u64 could wrap)
bool content_in_range(uint64_t first_block, uint64_t n_blocks) {
    return first_block <= CONTENT_MAX_BLOCK && n_blocks <= CONTENT_MAX_BLOCK &&
           first_block + n_blocks <= CONTENT_MAX_BLOCK;
}
constexpr void content_layout(Cursor& c, const Params& p, Fields& f) {
    c.magic("FRCCTXT1", "compact content: bad magic");
    c.k_N(p, "compact content: k, N do not match the context params");
    c.u64(f.first_block);
    c.u64(f.count);
    c.need([&] { return f.count == (f.len - CONTENT_HEADER) / 8; },
           "compact content: n_blocks does not match the length");
    c.need([&] { return content_in_range(f.first_block, f.count); }, CONTENT_RANGE);
    c.need([&] { return !f.radix || f.count % 4 == 0; }, "compact content: a string is 4 blocks per character");
    c.key(f.mask_key);
}

const char NEEDLE_LENGTH[] = "needle: length is not 64 + 16 m N (fr_needle_size)";
const char NEEDLE_RANGE[] = "needle: 1 <= m <= 64";
constexpr void needle_layout(Cursor& c, const Params& p, Fields& f) {
    c.magic("FRNEEDL1", "needle: bad magic");
    c.k_N(p, "needle: k, N do not match the context params");
    c.u64(f.count);
    c.need([&] { return f.count >= 1 && f.count <= NEEDLE_MAX_CHARS; }, NEEDLE_RANGE);
    c.need([&] { return f.len == needle_blob_size(p, (size_t)f.count); }, NEEDLE_LENGTH);
    c.key(f.mask_key);
    c.zeros(8, "needle: reserved bytes are not zero");
}

const char NEEDLE_BYTES_MAGIC[] = "FRNEEDB1";
const char NEEDLE_BYTES_LENGTH[] = "byte needle: length is not 64 + 8 ceil(256 m / N) N (fr_needle_bytes_size)";
constexpr void needle_bytes_layout(Cursor& c, const Params& p, Fields& f) {
    c.magic(NEEDLE_BYTES_MAGIC, "byte needle: bad magic");
    c.k_N(p, "byte needle: k, N do not match the context params");
    c.u64(f.count);
    c.need([&] { return f.count >= 1 && f.count <= NEEDLE_MAX_CHARS; }, NEEDLE_RANGE);
    c.need([&] { return f.len == needle_bytes_blob_size(p, (size_t)f.count); }, NEEDLE_BYTES_LENGTH);
    c.key(f.mask_key);
    c.zeros(8, "byte needle: reserved bytes are not zero");
}

using Layout = void (*)(Cursor&, const Params&, Fields&);
constexpr size_t header_bytes(Layout layout) {
    Cursor c;
    Params p;
    Fields f;
    layout(c, p, f);
    return c.n;
}
static_assert(header_bytes(compact_layout) == COMPACT_HEADER && header_bytes(pk_layout) == PK_HEADER &&
              header_bytes(pk_compact_layout) == PKC_HEADER && header_bytes(packed_result_layout) == PKRES_HEADER &&
              header_bytes(packed_compact_layout) == PKCRES_HEADER && header_bytes(content_layout) == CONTENT_HEADER &&
              header_bytes(needle_layout) == NEEDLE_HEADER && header_bytes(needle_bytes_layout) == NEEDLE_HEADER);

void write(Layout layout, const Params& p, Fields f, uint8_t* out) {
    Cursor c{nullptr, out};
    layout(c, p, f);
}
// the fields of a blob of at least the header's bytes, or the layout's refusal
Fields read(Layout layout, const Params& p, const uint8_t* blob, size_t len, bool radix = false) {
    Cursor c{blob};
    Fields f{0, 0, {}, len, radix};
    layout(c, p, f);
    return f;
}

}  // namespace

// ---------------------------------------------------------------- compact server key
size_t compact_size(const Params& p) { return COMPACT_HEADER + 8 * (compact_ksk_bodies(p) + compact_bsk_bodies(p)); }

RngKey check_compact(const Params& p, const uint8_t* blob, size_t len) {
    need(p.ring == FR_RING_FFT, "compact server key: FFT ring only");
    need(blob && len == compact_size(p),
         "compact server key: length does not match the context params (fr_server_key_compact_size)");
    return read(compact_layout, p, blob, len).mask_key;
}

void pack_compact(const Params& p, const RngKey& mask_key, const std::vector<uint64_t>& ksk,
                  const std::vector<uint64_t>& bsk, uint8_t* out) {
    need(p.ring == FR_RING_FFT, "compact server key: FFT ring only");
    const size_t rows = compact_ksk_bodies(p), n = (size_t)p.n, N = (size_t)p.N, kp1 = (size_t)p.k + 1;
    const size_t brows = p.bsk_ggsw() * kp1;
    need(ksk.size() == rows * (n + 1) && bsk.size() == p.bsk_len(), "compact server key: key array sizes");
    write(compact_layout, p, {0, 0, mask_key}, out);
    uint8_t* o = out + COMPACT_HEADER;
    for (size_t row = 0; row < rows; ++row, o += 8) std::memcpy(o, &ksk[row * (n + 1) + n], 8);
    for (size_t q = 0; q < brows; ++q, o += 8 * N) std::memcpy(o, &bsk[(q * kp1 + (kp1 - 1)) * N], 8 * N);
}

RngKey expand_compact(const Params& p, const uint8_t* blob, size_t len, std::vector<uint64_t>& ksk,
                      std::vector<uint64_t>& bsk) {
    const RngKey mask_key = check_compact(p, blob, len);
    const size_t rows = compact_ksk_bodies(p), n = (size_t)p.n, N = (size_t)p.N, k = (size_t)p.k, kp1 = k + 1;
    const size_t brows = p.bsk_ggsw() * kp1;
    const uint8_t* kb = blob + COMPACT_HEADER;
    const uint8_t* bb = kb + 8 * rows;
    ksk.resize(rows * (n + 1));
    bsk.resize(p.bsk_len());
    parallel_for((int)rows, [&](int row) {
        Rng rm(mask_key, STREAM_KSK_MASK);
        uint64_t* o = ksk.data() + (size_t)row * (n + 1);
        for (size_t t = 0; t < n; ++t) o[t] = rm.u64((uint64_t)row * n + t);
        std::memcpy(o + n, kb + 8 * (size_t)row, 8);
    });
    parallel_for((int)brows, [&](int q) {
        Rng rm(mask_key, STREAM_BSK_MASK);
        uint64_t* o = bsk.data() + (size_t)q * kp1 * N;
        for (size_t t = 0; t < k * N; ++t) o[t] = rm.u64((uint64_t)q * k * N + t);
        std::memcpy(o + k * N, bb + 8 * (size_t)q * N, 8 * N);
    });
    return mask_key;
}

// ---------------------------------------------------------------- packing key
void write_pk_header(const Params& p, uint8_t* out) { write(pk_layout, p, {}, out); }

void check_pk_blob(const Params& p, const uint8_t* blob, size_t len) {
    need(blob && len == pk_blob_size(p), "packing key: length does not match the context params (fr_packing_key_size)");
    read(pk_layout, p, blob, len);
}

// ---------------------------------------------------------------- compact packing key
void write_pk_compact_header(const Params& p, const RngKey& mask_key, uint8_t* out) {
    write(pk_compact_layout, p, {0, 0, mask_key}, out);
}

RngKey check_pk_compact(const Params& p, const uint8_t* blob, size_t len) {
    need(blob && len == pk_compact_size(p),
         "compact packing key: length does not match the context params (fr_packing_key_compact_size)");
    return read(pk_compact_layout, p, blob, len).mask_key;
}

void pack_pk_compact(const Params& p, const uint64_t* rows, uint8_t* planes) {
    const size_t R = pk_rows(p), N = (size_t)p.N, W = pk_row_words(p), kN = (size_t)p.k * N;
    uint8_t* lo = planes + 4 * R * N;
    parallel_for((int)R, [&](int r) {
        const uint64_t* body = rows + (size_t)r * W + kN;
        for (size_t t = 0; t < N; ++t) {
            const uint64_t b40 = body[t] >> PKC_DROP_BITS;
            put_le32(planes + 4 * ((size_t)r * N + t), (uint32_t)(b40 >> 8));
            lo[(size_t)r * N + t] = (uint8_t)b40;
        }
    });
}

RngKey expand_pk_compact(const Params& p, const uint8_t* blob, size_t len, std::vector<uint64_t>& rows) {
    const RngKey mask_key = check_pk_compact(p, blob, len);
    const size_t R = pk_rows(p), N = (size_t)p.N, W = pk_row_words(p), kN = (size_t)p.k * N;
    const uint8_t* hi = blob + PKC_HEADER;
    const uint8_t* lo = hi + 4 * R * N;
    rows.resize(pk_len(p));
    parallel_for((int)R, [&](int r) {
        Rng rm(mask_key, STREAM_PKSK_MASK);
        uint64_t* o = rows.data() + (size_t)r * W;
        for (size_t t = 0; t < kN; ++t) o[t] = rm.u64((uint64_t)r * kN + t);
        for (size_t t = 0; t < N; ++t) {
            const uint64_t b40 = ((uint64_t)get_le32(hi + 4 * ((size_t)r * N + t)) << 8) | lo[(size_t)r * N + t];
            o[kN + t] = b40 << PKC_DROP_BITS;
        }
    });
    return mask_key;
}

// ---------------------------------------------------------------- packed results
void write_packed_result(const Params& p, size_t n, const uint64_t* words, uint8_t* out) {
    write(packed_result_layout, p, {n}, out);
    for (size_t t = 0; t < pk_row_words(p); ++t) put_le64(out + PKRES_HEADER + 8 * t, words[t]);
}

size_t check_packed_result(const Params& p, const uint8_t* blob, size_t len) {
    need(blob && len == packed_result_size(p), "packed result: length is not 24 + 8 (k+1) N (fr_packed_result_size)");
    return (size_t)read(packed_result_layout, p, blob, len).count;
}

void write_packed_compact(const Params& p, size_t n, const uint16_t* values, uint8_t* out) {
    write(packed_compact_layout, p, {n}, out);
    for (size_t t = 0; t < packed_compact_values(p, n); ++t) {
        out[PKCRES_HEADER + 2 * t] = (uint8_t)values[t];
        out[PKCRES_HEADER + 2 * t + 1] = (uint8_t)(values[t] >> 8);
    }
}

void compress_packed(const Params& p, size_t n, const uint64_t* words, uint8_t* out) {
    need(n >= 1 && n <= (size_t)p.N, "compact packed result: n outside 1..N");
    // the body's first n coefficients follow the masks in the words as they do in the blob
    std::vector<uint16_t> v(packed_compact_values(p, n));
    for (size_t t = 0; t < v.size(); ++t) v[t] = packed_round16(words[t]);
    write_packed_compact(p, n, v.data(), out);
}

size_t check_packed_compact(const Params& p, const uint8_t* blob, size_t len) {
    need(blob && len >= PKCRES_HEADER, PKCRES_LENGTH);
    return (size_t)read(packed_compact_layout, p, blob, len).count;
}

size_t expand_packed_compact(const Params& p, const uint8_t* blob, size_t len, uint64_t* words) {
    const size_t n = check_packed_compact(p, blob, len), sent = packed_compact_values(p, n);
    for (size_t t = 0; t < pk_row_words(p); ++t) {
        const uint8_t* v = blob + PKCRES_HEADER + 2 * t;
        words[t] = t < sent ? ((uint64_t)v[0] | ((uint64_t)v[1] << 8)) << PKCRES_DROP : 0;
    }
    return n;
}

// ---------------------------------------------------------------- compact content
size_t content_blob_size(size_t n_blocks) {
    need(n_blocks <= CONTENT_MAX_BLOCK, "compact content: more than 2^40 blocks");
    return CONTENT_HEADER + 8 * n_blocks;
}

void check_content_range(uint64_t first_block, uint64_t n_blocks) {
    need(content_in_range(first_block, n_blocks), CONTENT_RANGE);
}

void write_content_header(const Params& p, uint64_t first_block, size_t n_blocks, const RngKey& mask_key,
                          uint8_t* out) {
    write(content_layout, p, {n_blocks, first_block, mask_key}, out);
}

ContentBlob check_content_blob(const Params& p, const uint8_t* blob, size_t len, bool radix) {
    need(blob && len >= CONTENT_HEADER && (len - CONTENT_HEADER) % 8 == 0,
         "compact content: length is not 64 + 8 n_blocks (fr_compact_content_size)");
    const Fields f = read(content_layout, p, blob, len, radix);
    return ContentBlob{f.mask_key, f.first_block, (size_t)f.count, blob + CONTENT_HEADER};
}

void expand_content(const Params& p, const uint8_t* blob, size_t len, uint64_t* out) {
    const ContentBlob c = check_content_blob(p, blob, len, false);
    const uint64_t big = (uint64_t)p.big();
    Rng rm(c.mask_key, STREAM_ENC_MASK);
    for (size_t q = 0; q < c.n_blocks; ++q) {
        uint64_t* o = out + q * (big + 1);
        const uint64_t qb = c.first_block + q;
        for (uint64_t t = 0; t < big; ++t) o[t] = rm.u64(qb * big + t);
        o[big] = get_le64(c.bodies + 8 * q);
    }
}

// ---------------------------------------------------------------- the needle
size_t needle_blob_size(const Params& p, size_t m) {
    need(m >= 1 && m <= NEEDLE_MAX_CHARS, NEEDLE_RANGE);
    return NEEDLE_HEADER + 16 * m * (size_t)p.N;
}

void write_needle_header(const Params& p, size_t m, const RngKey& mask_key, uint8_t* out) {
    write(needle_layout, p, {m, 0, mask_key}, out);
}

NeedleBlob check_needle_blob(const Params& p, const uint8_t* blob, size_t len) {
    need(p.ring == FR_RING_FFT, "private search: FFT ring only");
    need(blob && len >= NEEDLE_HEADER, NEEDLE_LENGTH);
    const Fields f = read(needle_layout, p, blob, len);
    return NeedleBlob{f.mask_key, (size_t)f.count, blob + NEEDLE_HEADER};
}

void expand_needle(const Params& p, const uint8_t* blob, size_t len, uint64_t* out) {
    const NeedleBlob nb = check_needle_blob(p, blob, len);
    const size_t k = (size_t)p.k, N = (size_t)p.N;
    parallel_for((int)(2 * nb.m), [&](int q) {
        Rng rm(nb.mask_key, STREAM_NEEDLE_MASK);
        uint64_t* o = out + (size_t)q * (k + 1) * N;
        for (size_t t = 0; t < k * N; ++t) o[t] = rm.u64((uint64_t)q * k * N + t);
        for (size_t t = 0; t < N; ++t) o[k * N + t] = get_le64(nb.bodies + 8 * ((size_t)q * N + t));
    });
}

// ---------------------------------------------------------------- the byte-table needle
size_t needle_bytes_blob_size(const Params& p, size_t m) {
    need(m >= 1 && m <= NEEDLE_MAX_CHARS, NEEDLE_RANGE);
    need(p.N >= 256 && p.N % 256 == 0, "byte needle: N is not a multiple of 256");
    return NEEDLE_HEADER + 8 * needle_bytes_selectors(p, m) * (size_t)p.N;
}

bool is_needle_bytes_blob(const uint8_t* blob, size_t len) {
    return blob && len >= 8 && !std::memcmp(blob, NEEDLE_BYTES_MAGIC, 8);
}

void write_needle_bytes_header(const Params& p, size_t m, const RngKey& mask_key, uint8_t* out) {
    write(needle_bytes_layout, p, {m, 0, mask_key}, out);
}

NeedleBlob check_needle_bytes_blob(const Params& p, const uint8_t* blob, size_t len) {
    need(p.ring == FR_RING_FFT, "private search: FFT ring only");
    need(p.N >= 256 && p.N % 256 == 0, "byte needle: N is not a multiple of 256");
    need(blob && len >= NEEDLE_HEADER, NEEDLE_BYTES_LENGTH);
    const Fields f = read(needle_bytes_layout, p, blob, len);
    return NeedleBlob{f.mask_key, (size_t)f.count, blob + NEEDLE_HEADER};
}

void expand_needle_bytes(const Params& p, const uint8_t* blob, size_t len, uint64_t* out) {
    const NeedleBlob nb = check_needle_bytes_blob(p, blob, len);
    const size_t k = (size_t)p.k, N = (size_t)p.N;
    parallel_for((int)needle_bytes_selectors(p, nb.m), [&](int q) {
        Rng rm(nb.mask_key, STREAM_NEEDLE_BYTES_MASK);
        uint64_t* o = out + (size_t)q * (k + 1) * N;
        for (size_t t = 0; t < k * N; ++t) o[t] = rm.u64((uint64_t)q * k * N + t);
        for (size_t t = 0; t < N; ++t) o[k * N + t] = get_le64(nb.bodies + 8 * ((size_t)q * N + t));
    });
}

}  // namespace fr
