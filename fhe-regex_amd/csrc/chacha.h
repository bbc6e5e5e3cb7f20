// ChaCha20 block function (RFC 8439 rounds; 256-bit key, nonce = stream,
// 64-bit block counter), shared by the host key generator (keys.cpp) and the
// device key generator (keygen.hip), so both draw the same words for the same
// (key, stream, index).  Word pair (2q, 2q+1) of block b is u64 number 8b + q.
#pragma once
#include <cstdint>

#include "common.h"

namespace fr {

// The generator key: ChaCha20 state words 4..11, little endian.  Every random
// draw of the library (client key, KSK/BSK masks and noise, encryption masks and
// noise) is a function of one RngKey, a stream id and an index.  A kernel takes
// it by value: the argument is wave-uniform, so the words live in scalar
// registers and never reach global memory.
struct RngKey {
    uint32_t w[8];

    // the reproducible keys of tests, benchmarks and multi-rank keygen: 64 bits
    // of seed and six fixed words (the first 192 fractional bits of pi)
    FR_HD static RngKey from_seed(uint64_t seed) {
        return RngKey{{(uint32_t)seed, (uint32_t)(seed >> 32), 0x243F6A88u, 0x85A308D3u, 0x13198A2Eu, 0x03707344u,
                       0xA4093822u, 0x299F31D0u}};
    }
    FR_HD static RngKey from_bytes(const uint8_t b[32]) {
        RngKey k;
        for (int i = 0; i < 8; ++i)
            k.w[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) |
                     ((uint32_t)b[4 * i + 3] << 24);
        return k;
    }
    // 32 bytes of the OS CSPRNG (getrandom(2)), a fresh key per call; throws
    // Error(FR_ERR_RNG) if the OS gives none, never a weaker source (keys.cpp)
    static RngKey from_os();
};
// zeroes a host copy of a key (not optimised away)
void wipe_key(RngKey& k);

FR_HD uint32_t chacha_rotl(uint32_t a, int b) { return (a << b) | (a >> (32 - b)); }

FR_HD void chacha_qr(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d) {
    a += b; d ^= a; d = chacha_rotl(d, 16);
    c += d; b ^= c; b = chacha_rotl(b, 12);
    a += b; d ^= a; d = chacha_rotl(d, 8);
    c += d; b ^= c; b = chacha_rotl(b, 7);
}

// the input state is read from `key` again for the final addition, so no second
// copy of the key words is made
FR_HD void chacha_block(const RngKey& key, uint64_t stream, uint64_t counter, uint32_t out[16]) {
    const uint32_t c[4] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u};
    const uint32_t t[4] = {(uint32_t)counter, (uint32_t)(counter >> 32), (uint32_t)stream, (uint32_t)(stream >> 32)};
    uint32_t x[16];
    for (int i = 0; i < 4; ++i) x[i] = c[i];
    for (int i = 0; i < 8; ++i) x[4 + i] = key.w[i];
    for (int i = 0; i < 4; ++i) x[12 + i] = t[i];
    for (int i = 0; i < 10; ++i) {
        chacha_qr(x[0], x[4], x[8], x[12]); chacha_qr(x[1], x[5], x[9], x[13]);
        chacha_qr(x[2], x[6], x[10], x[14]); chacha_qr(x[3], x[7], x[11], x[15]);
        chacha_qr(x[0], x[5], x[10], x[15]); chacha_qr(x[1], x[6], x[11], x[12]);
        chacha_qr(x[2], x[7], x[8], x[13]); chacha_qr(x[3], x[4], x[9], x[14]);
    }
    for (int i = 0; i < 4; ++i) out[i] = x[i] + c[i];
    for (int i = 0; i < 8; ++i) out[4 + i] = x[4 + i] + key.w[i];
    for (int i = 0; i < 4; ++i) out[12 + i] = x[12 + i] + t[i];
}

}  // namespace fr
