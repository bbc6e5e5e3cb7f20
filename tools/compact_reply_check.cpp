// Stand-alone host check of the compact packed result's blob functions (keys.h: compress_packed,
// check_packed_compact, expand_packed_compact) for a sanitized build; own main, no device, no
// library:
//
//   $ROCM/llvm/bin/clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iinclude -Ifhe-regex_amd/csrc tools/compact_reply_check.cpp fhe-regex_amd/csrc/keys.cpp \
//       -lpthread -o compact_reply_check && ./compact_reply_check
//
// At both FFT points and n = 1, 3, 33, N, on heap buffers of exactly the sizes the functions are
// documented to touch: words -> blob -> words gives ((x + 2^47) >> 48) << 48 on the k N + n sent
// coefficients and zero past them; every header byte, flipped, and every wrong length is refused
// with FR_ERR_INVALID.
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
        check_packed_compact(p, b, len);
    } catch (const Error& e) {
        return e.code == FR_ERR_INVALID;
    }
    return false;
}

int main() {
    for (int point = 0; point < 2; ++point) {
        Params p;
        if (point) p.k = 2, p.N = 1024;
        const size_t W = pk_row_words(p), N = (size_t)p.N;
        std::vector<uint64_t> words(W);
        for (size_t i = 0; i < W; ++i) words[i] = (i + 1) * 0x9E3779B97F4A7C15ULL;
        words[0] = ((uint64_t)0xFFFF << 48) + ((uint64_t)1 << 47);  // rounds up and wraps to 0
        words[1] = ((uint64_t)1 << 47) - 1;                         // rounds down to 0
        for (size_t n : {(size_t)1, (size_t)3, (size_t)33, N}) {
            std::vector<uint8_t> blob(packed_compact_size(p, n));
            compress_packed(p, n, words.data(), blob.data());
            if (check_packed_compact(p, blob.data(), blob.size()) != n) return puts("n"), 1;
            std::vector<uint64_t> back(W, ~(uint64_t)0);
            expand_packed_compact(p, blob.data(), back.data());
            const size_t sent = (size_t)p.big() + n;
            for (size_t t = 0; t < W; ++t) {
                const uint64_t want = t < sent ? ((words[t] + ((uint64_t)1 << 47)) >> 48) << 48 : 0;
                if (back[t] != want) return printf("word %zu at n = %zu\n", t, n), 1;
            }
            if (back[0] != 0 || back[1] != 0) return puts("edge"), 1;
            for (size_t at = 0; at < PKCRES_HEADER; ++at) {
                blob[at] ^= 0x10;
                if (!refused(p, blob.data(), blob.size())) return printf("accepted byte %zu\n", at), 1;
                blob[at] ^= 0x10;
            }
            if (!refused(p, blob.data(), blob.size() - 1) || !refused(p, blob.data(), PKCRES_HEADER - 1) ||
                !refused(p, blob.data(), 0) || !refused(p, nullptr, blob.size()))
                return puts("length"), 1;
            std::vector<uint8_t> longer(blob);
            longer.push_back(0);
            if (!refused(p, longer.data(), longer.size())) return puts("long"), 1;
            if (refused(p, blob.data(), blob.size())) return puts("good blob refused"), 1;
        }
        bool threw = false;
        try {
            std::vector<uint8_t> blob(packed_compact_size(p, N));
            compress_packed(p, N + 1, words.data(), blob.data());
        } catch (const Error& e) {
            threw = e.code == FR_ERR_INVALID;
        }
        if (!threw) return puts("n = N + 1 compressed"), 1;
        printf("point %d ok\n", point);
    }
    return 0;
}
