// Stand-alone host check of the find lowerings (lower.h: compile_needle, compile_needle_clear, eval_program_parts) for
// a sanitized build; own main, no device, no library (the needle's blob: wire_check.cpp):
//
//   $ROCM/llvm/bin/clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iinclude -Ifhe-regex_amd/csrc tools/needle_check.cpp fhe-regex_amd/csrc/lower.cpp \
//       fhe-regex_amd/csrc/regex.cpp fhe-regex_amd/csrc/merged.cpp -lpthread -o needle_check && ./needle_check
//
// The lowered find of every (n_chars, m) up to 20 x 20, in plaintext, evaluates to a plain
// search's answer: over encrypted content (selector gates) and over clear content (extract-sums).
#include <cstdio>
#include <vector>

#include "lower.h"

namespace fr {
void set_last_error(const std::string&) {}
}  // namespace fr
using namespace fr;

// the lowered programs of one (content, needle) against a plain search: what differs, or null
static const char* check(Program (*compile)(size_t, size_t, size_t, size_t, bool), const std::vector<uint8_t>& content,
                         const std::vector<uint16_t>& masks) {
    const size_t n = content.size(), m = masks.size() / 2;
    std::vector<int> starts, one;
    eval_program_parts(compile(n, m, 0, n + 1, true), content.data(), n, starts, masks.data(), 2 * m);
    const int any = eval_program_parts(compile(n, m, 0, n + 1, false), content.data(), n, one, masks.data(), 2 * m);
    int want_any = 0;
    for (size_t p = 0; p <= n; ++p) {
        int ok = p + m <= n;
        for (size_t i = 0; ok && i < m; ++i)
            ok = ((masks[2 * i] >> (content[p + i] & 15)) & 1) && ((masks[2 * i + 1] >> (content[p + i] >> 4)) & 1);
        if (starts.at(p) != ok) return "a start";
        want_any |= ok;
    }
    return any != want_any ? "the OR" : nullptr;
}

int main() {
    uint64_t x = 88172645463325252ULL;
    auto rnd = [&]() { return x ^= x << 13, x ^= x >> 7, x ^= x << 17, x; };
    for (size_t n = 1; n <= 20; ++n)
        for (size_t m = 1; m <= 20; ++m) {
            std::vector<uint8_t> content(n);
            for (auto& c : content) c = (uint8_t)("abAB"[rnd() % 4]);
            std::vector<uint16_t> masks(2 * m);
            for (size_t i = 0; i < m; ++i) {
                const uint8_t c = (uint8_t)("abAB"[rnd() % 4]);
                const bool wild = rnd() % 5 == 0;
                masks[2 * i] = wild ? 0xFFFF : (uint16_t)(1u << (c & 15));
                masks[2 * i + 1] = wild ? 0xFFFF : (uint16_t)(1u << (c >> 4));
            }
            for (const auto compile : {compile_needle, compile_needle_clear})
                if (const char* bad = check(compile, content, masks)) return printf("%s n=%zu m=%zu\n", bad, n, m), 1;
        }
    printf("needle_check: ok\n");
    return 0;
}
