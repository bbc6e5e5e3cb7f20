/* Stand-alone fuzz of the compact content blob parser on a host-only context, for a
 * sanitized build of the library (make -C fhe-regex_amd asan):
 *
 *   CL=$ROCM/llvm/bin/clang; RT=$(dirname $($CL -print-file-name=libclang_rt.asan-x86_64.so))
 *   $CL -g -fsanitize=address,undefined -shared-libsan -Iinclude tools/compact_content_fuzz.c \
 *       -Lfhe-regex_amd/build-asan -lfheregex -Wl,-rpath,$PWD/fhe-regex_amd/build-asan -Wl,-rpath,$RT \
 *       -Wl,-rpath-link,$ROCM/lib -o compact_content_fuzz
 *   ./compact_content_fuzz tests/golden/client_key [iterations]
 *
 * It encrypts strings and blocks to blobs, expands them, then mutates header bytes, body
 * bytes and the length and checks every return code: a mutated blob is refused with
 * FR_ERR_INVALID or expands (into a buffer of exactly n_blocks * (kN + 1) words, so that a
 * write past it is an ASan report); the uploads of a host-only context answer
 * FR_ERR_INVALID for a bad blob and FR_ERR_NO_DEVICE for a good one.  Exit status 0 and a
 * summary line, or 1 at the first unexpected code. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fheregex.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(void) { /* xorshift64* */
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}

#define CHECK(cond)                                                                         \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            fprintf(stderr, "line %d: %s failed (%s)\n", __LINE__, #cond, fr_last_error()); \
            return 1;                                                                       \
        }                                                                                   \
    } while (0)

static int run_point(int32_t k, int32_t N, int32_t ring, const uint8_t* ck, size_t ck_len, long iters,
                     long* accepted, long* refused) {
    fr_params p;
    CHECK(fr_default_params(&p) == FR_OK);
    p.k = k, p.N = N, p.ring = ring;
    fr_ctx *client = NULL, *server = NULL;
    CHECK(fr_ctx_create(&p, -1, &client) == FR_OK && fr_ctx_create(&p, -1, &server) == FR_OK);
    CHECK(fr_load_client_key(client, ck, ck_len) == FR_OK);
    const size_t L = (size_t)k * N + 1;
    uint8_t key[32];
    for (int i = 0; i < 32; ++i) key[i] = (uint8_t)(rnd() >> 24);

    /* a string blob and a block blob with a counter above 32 bits */
    const char* s = "fuzz me: abc";
    size_t need = 0, wrote = 0, bytes = 0;
    CHECK(fr_encrypt_str_compact_keyed(client, s, strlen(s), key, NULL, 0, &need) == FR_OK);
    CHECK(fr_compact_content_size(client, 4 * strlen(s), &bytes) == FR_OK && bytes == need);
    uint8_t* sblob = malloc(need);
    CHECK(fr_encrypt_str_compact_keyed(client, s, strlen(s), key, sblob, need - 1, &wrote) == FR_ERR_INVALID);
    CHECK(fr_encrypt_str_compact_keyed(client, s, strlen(s), key, sblob, need, &wrote) == FR_OK && wrote == need);
    CHECK(fr_encrypt_str_compact_keyed(server, s, strlen(s), key, sblob, need, &wrote) == FR_ERR_NO_KEY);
    CHECK(fr_encrypt_str_compact_keyed(client, "caf\xc3\xa9", 5, key, NULL, 0, &wrote) == FR_ERR_NON_ASCII);
    const uint8_t msgs[5] = {0, 15, 7, 8, 3};
    size_t bneed = 0;
    CHECK(fr_encrypt_blocks_compact_keyed(client, msgs, 5, NULL, (1ull << 33) + 5, NULL, 0, &bneed) == FR_OK);
    uint8_t* bblob = malloc(bneed);
    CHECK(fr_encrypt_blocks_compact_keyed(client, msgs, 5, NULL, (1ull << 33) + 5, bblob, bneed, &wrote) == FR_OK);

    /* expansion into an exact-size buffer, decryption */
    size_t nb = 0;
    CHECK(fr_expand_compact_content(server, sblob, need, NULL, 0, &nb) == FR_OK && nb == 4 * strlen(s));
    uint64_t* out = malloc(8 * nb * L);
    CHECK(fr_expand_compact_content(server, sblob, need, out, nb * L - 1, &nb) == FR_ERR_INVALID);
    CHECK(fr_expand_compact_content(server, sblob, need, out, nb * L, &nb) == FR_OK);
    for (size_t i = 0; i < strlen(s); ++i) {
        uint64_t v = 0;
        CHECK(fr_decrypt_radix(client, out + 4 * i * L, &v) == FR_OK && v == (uint64_t)s[i]);
    }
    free(out);
    out = malloc(8 * 5 * L);
    CHECK(fr_expand_compact_content(server, bblob, bneed, out, 5 * L, &nb) == FR_OK && nb == 5);
    for (int i = 0; i < 5; ++i) {
        uint32_t v = 0;
        CHECK(fr_decode_block(client, out + i * L, &v) == FR_OK && v == msgs[i]);
    }
    free(out);
    fr_ct h[256];
    size_t n = 0;
    CHECK(fr_upload_compact_str(server, sblob, need, h, 256, &n) == FR_ERR_NO_DEVICE);
    CHECK(fr_upload_compact_str(server, bblob, bneed, h, 256, &n) == FR_ERR_INVALID); /* 5 % 4 != 0 */
    CHECK(fr_upload_compact_blocks(server, bblob, bneed, h, 256, &n) == FR_ERR_NO_DEVICE);

    /* mutations: 1..3 bytes anywhere (header-heavy), and / or a changed length */
    for (long it = 0; it < iters; ++it) {
        const uint8_t* src = it & 1 ? sblob : bblob;
        const size_t slen = it & 1 ? need : bneed;
        size_t len = slen;
        const unsigned kind = (unsigned)(rnd() % 3);
        if (kind != 1) {
            const size_t cuts[] = {1, 7, 8, 9, 63, 64, (size_t)(rnd() % (slen + 1))};
            const size_t cut = cuts[rnd() % 7];
            len = rnd() & 1 ? (cut <= slen ? slen - cut : 0) : slen + cut;
        }
        uint8_t* m = malloc(len ? len : 1); /* exact size: a read past len is an ASan report */
        for (size_t i = 0; i < len; ++i) m[i] = i < slen ? src[i] : (uint8_t)rnd();
        if (kind != 0 && len)
            for (int c = 1 + (int)(rnd() % 3); c > 0; --c) {
                const size_t pos = (rnd() % 4 ? rnd() % 64 : rnd() % len) % len;
                m[pos] = (uint8_t)rnd();
            }
        size_t mb = 0;
        int rc = fr_expand_compact_content(server, m, len, NULL, 0, &mb);
        CHECK(rc == FR_OK || rc == FR_ERR_INVALID);
        if (rc == FR_OK) {
            CHECK(len == 64 + 8 * mb);
            uint64_t* o = malloc(mb ? 8 * mb * L : 8);
            CHECK(fr_expand_compact_content(server, m, len, o, mb * L, &mb) == FR_OK);
            for (size_t q = 0; q < mb; ++q) CHECK(memcmp(o + q * L + (L - 1), m + 64 + 8 * q, 8) == 0);
            free(o);
            CHECK(fr_upload_compact_blocks(server, m, len, h, 256, &n) == FR_ERR_NO_DEVICE);
            CHECK(fr_upload_compact_str(server, m, len, h, 256, &n) == (mb % 4 ? FR_ERR_INVALID : FR_ERR_NO_DEVICE));
            ++*accepted;
        } else {
            CHECK(fr_upload_compact_blocks(server, m, len, h, 256, &n) == FR_ERR_INVALID);
            CHECK(fr_upload_compact_str(server, m, len, h, 256, &n) == FR_ERR_INVALID);
            ++*refused;
        }
        free(m);
    }
    free(sblob);
    free(bblob);
    CHECK(fr_ctx_destroy(client) == FR_OK && fr_ctx_destroy(server) == FR_OK);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s CLIENT_KEY_FILE [iterations]\n", argv[0]);
        return 2;
    }
    const long iters = argc > 2 ? atol(argv[2]) : 2000;
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t* ck = malloc((size_t)sz);
    if (fread(ck, 1, (size_t)sz, f) != (size_t)sz) return 2;
    fclose(f);
    long accepted = 0, refused = 0;
    const int32_t points[3][3] = {{1, 2048, FR_RING_FFT}, {2, 1024, FR_RING_FFT}, {1, 2048, FR_RING_RNS}};
    for (int i = 0; i < 3; ++i)
        if (run_point(points[i][0], points[i][1], points[i][2], ck, (size_t)sz, iters, &accepted, &refused)) return 1;
    free(ck);
    printf("compact_content_fuzz ok: 3 points x %ld mutations, %ld expanded, %ld refused\n", iters, accepted, refused);
    return 0;
}
