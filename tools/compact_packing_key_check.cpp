// Stand-alone host check of the compact packing key's blob functions (keys.h: row generator,
// pack_pk_compact, check_pk_compact, expand_pk_compact) for a sanitized build; own main, no
// device, no library:
//
//   $ROCM/llvm/bin/clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iinclude -Ifhe-regex_amd/csrc tools/compact_packing_key_check.cpp fhe-regex_amd/csrc/keys.cpp \
//       -lpthread -o compact_packing_key_check && ./compact_packing_key_check
//
// At both FFT points: a key with generated first and last rows and arbitrary 40-bit bodies in
// between goes rows -> planes -> rows and comes back word for word; every header byte but the
// mask key's, flipped, and every wrong length is refused with FR_ERR_INVALID.
#include <cstdio>
#include <cstring>
#include <vector>

#include "keys.h"

namespace fr {
void set_last_error(const std::string&) {}
}  // namespace fr
using namespace fr;

static bool refused(const Params& p, const uint8_t* b, size_t len) {
    try {
        check_pk_compact(p, b, len);
    } catch (const Error& e) {
        return e.code == FR_ERR_INVALID;
    }
    return false;
}

int main() {
    for (int point = 0; point < 2; ++point) {
        Params p;
        if (point) p.k = 2, p.N = 1024;
        const RngKey K = RngKey::from_seed(77);
        const ClientKey ck = gen_client_key(p, K);
        const RngKey M = derive_mask_key(K);
        const size_t R = pk_rows(p), W = pk_row_words(p), N = p.N;
        // a key whose first and last rows are real and whose other bodies are arbitrary 40-bit words
        std::vector<uint64_t> rows(pk_len(p));
        for (size_t i = 0; i < rows.size(); ++i) rows[i] = (i * 0x9E3779B97F4A7C15ULL) & ~(uint64_t)0xFFFFFF;
        gen_packing_rows(p, ck, M, K, true, 0, 2, rows.data());
        gen_packing_rows(p, ck, M, K, true, R - 1, R, rows.data() + (R - 1) * W);
        std::vector<uint64_t> std_row(W);
        gen_packing_rows(p, ck, K, 0, 1, std_row.data());
        std::vector<uint8_t> blob(pk_compact_size(p));
        write_pk_compact_header(p, M, blob.data());
        pack_pk_compact(p, rows.data(), blob.data() + PKC_HEADER);
        std::vector<uint64_t> back;
        RngKey m2;
        expand_pk_compact(p, blob.data(), blob.size(), back, m2);
        if (std::memcmp(&m2, &M, sizeof M)) return puts("mask key"), 1;
        // bodies everywhere; masks where the rows were generated
        for (size_t r = 0; r < R; ++r)
            if (std::memcmp(&back[r * W + p.k * N], &rows[r * W + p.k * N], 8 * N)) return printf("body %zu\n", r), 1;
        for (size_t r : {(size_t)0, (size_t)1, R - 1})
            if (std::memcmp(&back[r * W], &rows[r * W], 8 * W)) return printf("row %zu\n", r), 1;
        // every header byte and both lengths
        for (size_t at = 0; at < PKC_HEADER; ++at) {
            if (at >= 56 && at < 88) continue;  // the mask key: any value is one
            blob[at] ^= 0x10;
            if (!refused(p, blob.data(), blob.size())) return printf("accepted byte %zu\n", at), 1;
            blob[at] ^= 0x10;
        }
        if (!refused(p, blob.data(), blob.size() - 1) || !refused(p, blob.data(), PKC_HEADER) ||
            !refused(p, blob.data(), 0) || !refused(p, nullptr, blob.size()))
            return puts("length"), 1;
        std::vector<uint8_t> longer(blob);
        longer.push_back(0);
        if (!refused(p, longer.data(), longer.size())) return puts("long"), 1;
        if (refused(p, blob.data(), blob.size())) return puts("good blob refused"), 1;
        printf("point %d ok: %zu bytes\n", point, blob.size());
    }
    return 0;
}
