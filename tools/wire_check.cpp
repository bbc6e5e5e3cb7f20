// Stand-alone host check of the wire layer (wire.h: the seven blobs' writers, checkers and
// expansions) for a sanitized build; own main, no device, no library:
//
//   $ROCM/llvm/bin/clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iinclude -Ifhe-regex_amd/csrc tools/wire_check.cpp fhe-regex_amd/csrc/wire.cpp \
//       fhe-regex_amd/csrc/keys.cpp -lpthread -o wire_check && ./wire_check
//
// At both FFT points, on heap buffers of exactly the documented sizes (a read or write past either
// end is a sanitizer report), per format: a round trip through the writer and the checker or the
// expansion; every checked header byte, flipped, and every wrong length refused with FR_ERR_INVALID
// (unchecked: a mask key's 32 bytes, any value being one, and the low five of a content blob's
// first_block, any block below 2^40 being one); the two FFT-only formats refused on the RNS ring.
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <vector>

#include "wire.h"

namespace fr {
void set_last_error(const std::string&) {}
}  // namespace fr
using namespace fr;

#define OK(cond, ...) \
    if (!(cond)) return printf(__VA_ARGS__), puts(""), false
using Bytes = std::unique_ptr<uint8_t[]>;
using Words = std::unique_ptr<uint64_t[]>;
using Check = std::function<void(const uint8_t*, size_t)>;

// the first `len` bytes of `src` (zeros past `have`) in a heap block of exactly `len`
static Bytes exact(const uint8_t* src, size_t have, size_t len) {
    Bytes b(new uint8_t[len ? len : 1]());
    std::memcpy(b.get(), src, len < have ? len : have);
    return b;
}
static bool refused(const Check& check, const uint8_t* b, size_t len) {
    try {
        check(b, len);
    } catch (const Error& e) {
        return e.code == FR_ERR_INVALID;
    }
    return false;
}
// the good blob is accepted; every header byte but those of the `free` ranges [lo, hi), flipped,
// and every wrong length is refused
static bool refusals(const char* name, const uint8_t* good, size_t len, size_t header,
                     const std::vector<std::pair<size_t, size_t>>& free, const Check& check) {
    Bytes b = exact(good, len, len);
    OK(!refused(check, b.get(), len), "%s: good blob refused", name);
    for (size_t at = 0; at < header; ++at) {
        bool checked = true;
        for (const auto& f : free) checked &= at < f.first || at >= f.second;
        b[at] ^= 0x10;
        OK(!checked || refused(check, b.get(), len), "%s: header byte %zu accepted", name, at);
        b[at] ^= 0x10;
    }
    for (size_t l : {(size_t)0, (size_t)8, header - 1, header, len - 8, len - 1, len + 1, len + 8})
        OK(l == len || refused(check, exact(good, len, l).get(), l), "%s: length %zu accepted", name, l);
    OK(refused(check, nullptr, len), "%s: null accepted", name);
    return true;
}
static uint64_t word(size_t i) { return (i + 1) * 0x9E3779B97F4A7C15ULL; }
static Params rns_ring(Params p) { return p.ring = FR_RING_RNS, p; }

static bool server_key(const Params& p) {
    // arbitrary arrays: the blob keeps their bodies, the expansion draws every mask from the mask key
    const RngKey M = derive_mask_key(RngKey::from_seed(5));
    const size_t rows = compact_ksk_bodies(p), n = (size_t)p.n, W = pk_row_words(p), kN = (size_t)p.big();
    std::vector<uint64_t> ksk(p.ksk_len()), bsk(p.bsk_len()), k2, b2;
    for (size_t i = 0; i < ksk.size(); ++i) ksk[i] = word(i);
    for (size_t i = 0; i < bsk.size(); ++i) bsk[i] = word(i + 7);
    const size_t len = compact_size(p);
    const Bytes blob(new uint8_t[len]);
    pack_compact(p, M, ksk, bsk, blob.get());
    const RngKey m2 = expand_compact(p, blob.get(), len, k2, b2);
    OK(!std::memcmp(&m2, &M, sizeof M) && k2.size() == ksk.size() && b2.size() == bsk.size(), "FRCSKEY1: expand");
    Rng km(M, STREAM_KSK_MASK), bm(M, STREAM_BSK_MASK);
    for (size_t r = 0; r < rows; ++r)
        OK(k2[r * (n + 1) + n] == ksk[r * (n + 1) + n] && k2[r * (n + 1)] == km.u64(r * n), "FRCSKEY1: ksk row %zu", r);
    for (size_t q = 0; q < bsk.size() / W; ++q)
        OK(!std::memcmp(&b2[q * W + kN], &bsk[q * W + kN], 8 * (size_t)p.N) &&
               b2[q * W + kN - 1] == bm.u64((q + 1) * kN - 1), "FRCSKEY1: bsk row %zu", q);
    OK(refused([&, rns = rns_ring(p)](const uint8_t* b, size_t l) { check_compact(rns, b, l); }, blob.get(), len),
       "FRCSKEY1: rns");
    return refusals("FRCSKEY1", blob.get(), len, COMPACT_HEADER, {{40, 72}},
                    [&](const uint8_t* b, size_t l) { check_compact(p, b, l); });
}

static bool content(const Params& p, const ClientKey& ck) {
    const RngKey K = RngKey::from_seed(9), M = derive_mask_key(K);
    const std::vector<uint8_t> msgs = {0, 15, 3, 9, 1, 2, 3, 0};
    const size_t L = (size_t)p.lwe_len(), first = 1000;
    const std::vector<uint8_t> v = encrypt_content_blob(p, ck, msgs.data(), msgs.size(), K, first);
    OK(v.size() == content_blob_size(msgs.size()) && v.size() == CONTENT_HEADER + 8 * msgs.size(), "FRCCTXT1: size");
    const Bytes blob = exact(v.data(), v.size(), v.size());
    Words got(new uint64_t[msgs.size() * L]), want(new uint64_t[msgs.size() * L]);
    expand_content(p, blob.get(), v.size(), got.get());
    encrypt_blocks(p, ck, msgs.data(), msgs.size(), M, K, first, want.get());
    OK(!std::memcmp(got.get(), want.get(), 8 * msgs.size() * L), "FRCCTXT1: expand");
    // a string is whole characters: 7 blocks are blocks only
    const std::vector<uint8_t> odd = encrypt_content_blob(p, ck, msgs.data(), 7, K, first);
    const Check str = [&](const uint8_t* b, size_t l) { check_content_blob(p, b, l, true); };
    const Check any = [&](const uint8_t* b, size_t l) { check_content_blob(p, b, l, false); };
    OK(!refused(str, blob.get(), v.size()) && !refused(any, odd.data(), odd.size()) &&
           refused(str, odd.data(), odd.size()), "FRCCTXT1: radix");
    return refusals("FRCCTXT1", v.data(), v.size(), CONTENT_HEADER, {{16, 21}, {32, 64}}, any);
}

static bool packing_keys(const Params& p, const ClientKey& ck) {
    const RngKey K = RngKey::from_seed(77), M = derive_mask_key(K);
    const size_t R = pk_rows(p), W = pk_row_words(p), N = p.N;
    // a key whose first and last rows are real and whose other bodies are arbitrary 40-bit words
    std::vector<uint64_t> rows(pk_len(p));
    for (size_t i = 0; i < rows.size(); ++i) rows[i] = word(i) & ~(uint64_t)0xFFFFFF;
    gen_packing_rows(p, ck, M, K, true, 0, 2, rows.data());
    gen_packing_rows(p, ck, M, K, true, R - 1, R, rows.data() + (R - 1) * W);
    Bytes full(new uint8_t[pk_blob_size(p)]);
    write_pk_header(p, full.get());
    std::memcpy(full.get() + PK_HEADER, rows.data(), 8 * rows.size());
    if (!refusals("FRPKKEY1", full.get(), pk_blob_size(p), PK_HEADER, {},
                  [&](const uint8_t* b, size_t l) { check_pk_blob(p, b, l); }))
        return false;
    Bytes blob(new uint8_t[pk_compact_size(p)]);
    write_pk_compact_header(p, M, blob.get());
    pack_pk_compact(p, rows.data(), blob.get() + PKC_HEADER);
    std::vector<uint64_t> back;
    const RngKey m2 = expand_pk_compact(p, blob.get(), pk_compact_size(p), back);
    OK(!std::memcmp(&m2, &M, sizeof M), "FRCPKEY1: mask key");
    // bodies everywhere; masks where the rows were generated
    for (size_t r = 0; r < R; ++r)
        OK(!std::memcmp(&back[r * W + p.k * N], &rows[r * W + p.k * N], 8 * N), "FRCPKEY1: body %zu", r);
    for (size_t r : {(size_t)0, (size_t)1, R - 1})
        OK(!std::memcmp(&back[r * W], &rows[r * W], 8 * W), "FRCPKEY1: row %zu", r);
    return refusals("FRCPKEY1", blob.get(), pk_compact_size(p), PKC_HEADER, {{56, 88}},
                    [&](const uint8_t* b, size_t l) { check_pk_compact(p, b, l); });
}

static bool packed_results(const Params& p) {
    const size_t W = pk_row_words(p), N = (size_t)p.N;
    Words words(new uint64_t[W]), back(new uint64_t[W]);
    for (size_t i = 0; i < W; ++i) words[i] = word(i);
    words[0] = ((uint64_t)0xFFFF << 48) + ((uint64_t)1 << 47);  // rounds up and wraps to 0
    words[1] = ((uint64_t)1 << 47) - 1;                         // rounds down to 0
    // (n = N: every bit of the count is checked; a smaller n has free low bits)
    Bytes full(new uint8_t[packed_result_size(p)]);
    write_packed_result(p, N, words.get(), full.get());
    OK(check_packed_result(p, full.get(), packed_result_size(p)) == N &&
           !std::memcmp(full.get() + PKRES_HEADER, words.get(), 8 * W), "FRPKRES1: round trip");
    if (!refusals("FRPKRES1", full.get(), packed_result_size(p), PKRES_HEADER, {},
                  [&](const uint8_t* b, size_t l) { check_packed_result(p, b, l); }))
        return false;
    for (size_t n : {(size_t)1, (size_t)3, (size_t)33, N}) {
        const size_t len = packed_compact_size(p, n), sent = packed_compact_values(p, n);
        Bytes blob(new uint8_t[len]);
        compress_packed(p, n, words.get(), blob.get());
        std::fill(back.get(), back.get() + W, ~(uint64_t)0);
        OK(expand_packed_compact(p, blob.get(), len, back.get()) == n, "FRCPRES1: n");
        for (size_t t = 0; t < W; ++t)
            OK(back[t] == (t < sent ? ((words[t] + ((uint64_t)1 << 47)) >> 48) << 48 : 0), "FRCPRES1: word %zu n %zu", t, n);
        OK(back[0] == 0 && back[1] == 0, "FRCPRES1: edge");
        if (!refusals("FRCPRES1", blob.get(), len, PKCRES_HEADER, {},
                      [&](const uint8_t* b, size_t l) { check_packed_compact(p, b, l); }))
            return false;
    }
    Bytes blob(new uint8_t[packed_compact_size(p, N)]);
    OK(refused([&](const uint8_t*, size_t) { compress_packed(p, N + 1, words.get(), blob.get()); }, nullptr, 0),
       "FRCPRES1: n = N + 1 compressed");
    return true;
}

static bool needle(const Params& p, const ClientKey& ck) {
    const size_t N = (size_t)p.N;
    for (size_t m : {(size_t)1, (size_t)3, (size_t)64}) {
        std::vector<uint16_t> masks(2 * m);
        for (size_t q = 0; q < 2 * m; ++q)
            masks[q] = (uint16_t)(q % 5 == 0 ? 0xFFFF : q % 5 == 1 ? 0 : 0x9E37u * (q + 1));
        const std::vector<uint8_t> v = encrypt_needle_blob(p, ck, masks.data(), m, RngKey::from_seed(11));
        OK(v.size() == needle_blob_size(p, m) && v.size() == NEEDLE_HEADER + 16 * m * N, "FRNEEDL1: size");
        const Bytes blob = exact(v.data(), v.size(), v.size());
        Words words(new uint64_t[needle_words(p, m)]);
        expand_needle(p, blob.get(), v.size(), words.get());
        std::vector<uint64_t> phase(N);
        for (size_t q = 0; q < 2 * m; ++q) {
            glwe_phase(p, ck, words.get() + q * (size_t)(p.k + 1) * N, phase.data());
            for (size_t t = 0; t < N; ++t) {
                const int64_t e = (int64_t)(phase[t] - needle_test_poly(p.N, (int)t, masks[q]));
                OK(e < (1 << 16) && e > -(1 << 16), "FRNEEDL1: phase m=%zu q=%zu t=%zu", m, q, t);
            }
        }
        if (!refusals("FRNEEDL1", v.data(), v.size(), NEEDLE_HEADER, {{24, 56}},
                      [&](const uint8_t* b, size_t l) { check_needle_blob(p, b, l); }))
            return false;
    }
    std::vector<uint8_t> v(needle_blob_size(p, 1));
    OK(refused([&, rns = rns_ring(p)](const uint8_t* b, size_t l) { check_needle_blob(rns, b, l); }, v.data(), v.size()),
       "FRNEEDL1: rns");
    return true;
}

int main() {
    for (int point = 0; point < 2; ++point) {
        Params p;
        if (point) p.k = 2, p.N = 1024;
        const ClientKey ck = gen_client_key(p, RngKey::from_seed(7));
        if (!server_key(p) || !content(p, ck) || !packing_keys(p, ck) || !packed_results(p) || !needle(p, ck)) return 1;
        printf("point %d ok\n", point);
    }
    return 0;
}
