// The host half of consensus/ethash, plain C++ with no HIP in it (g++ compiles it for
// tests/native/ethash_host_main.cpp): the epoch's sizes and seed, and the verification cache.
//
//   cache_size / dataset_size   algorithm.go:53-91, by calcCacheSize / calcDatasetSize: the highest prime
//                               row count below the linear bound.  The reference's 2,048-entry tables are
//                               that formula's values (algorithm_test.go:35-48) and are not copied in.
//   seed_hash                   algorithm.go:110-120
//   make_cache                  generateCache, algorithm.go:128-197: a sequential Keccak-512 fill, then three
//                               RandMemoHash rounds; the words come out little-endian.
//
// The cache stays on the host on purpose.  It is rows + 3 rows strictly dependent permutations (1.05 million
// at epoch 0): a CPU core runs them in under a second, and on the GPU the chain would occupy a single lane
// at a few hundred instructions per round with nothing to overlap.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "ethash_mod.h"

namespace gsv {
namespace ethash {

constexpr uint64_t EPOCH_LENGTH = 30000;
constexpr uint64_t CACHE_INIT_BYTES = 1ull << 24, CACHE_GROWTH_BYTES = 1ull << 17;
constexpr uint64_t DATASET_INIT_BYTES = 1ull << 30, DATASET_GROWTH_BYTES = 1ull << 23;
constexpr uint64_t HASH_BYTES = 64, MIX_BYTES = 128;
constexpr int CACHE_ROUNDS = 3;
// ModeTest (ethash.go:219-221, consensus.go:485-487)
constexpr uint64_t TEST_CACHE_BYTES = 1024, TEST_DATASET_BYTES = 32 * 1024;

inline bool is_prime(uint64_t n) {
    if (n < 2) return false;
    if (n < 4) return true;
    if ((n & 1) == 0) return false;
    for (uint64_t f = 3; f * f <= n; f += 2)
        if (n % f == 0) return false;
    return true;
}

inline uint64_t calc_cache_size(uint64_t epoch) {
    uint64_t size = CACHE_INIT_BYTES + CACHE_GROWTH_BYTES * epoch - HASH_BYTES;
    while (!is_prime(size / HASH_BYTES)) size -= 2 * HASH_BYTES;
    return size;
}

inline uint64_t calc_dataset_size(uint64_t epoch) {
    uint64_t size = DATASET_INIT_BYTES + DATASET_GROWTH_BYTES * epoch - MIX_BYTES;
    while (!is_prime(size / MIX_BYTES)) size -= 2 * MIX_BYTES;
    return size;
}

inline uint64_t cache_size(uint64_t block) { return calc_cache_size(block / EPOCH_LENGTH); }
inline uint64_t dataset_size(uint64_t block) { return calc_dataset_size(block / EPOCH_LENGTH); }

// ---- a portable 64-bit Keccak-f[1600] (crypto/sha3/keccakf.go) and the pre-FIPS sponge (pad 0x01 ... 0x80)
inline uint64_t rotl64(uint64_t v, int r) { return r ? (v << r) | (v >> (64 - r)) : v; }

inline void keccakf(uint64_t a[25]) {
    static const uint64_t RC[24] = {
        0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808AULL, 0x8000000080008000ULL,
        0x000000000000808BULL, 0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL,
        0x000000000000008AULL, 0x0000000000000088ULL, 0x0000000080008009ULL, 0x000000008000000AULL,
        0x000000008000808BULL, 0x800000000000008BULL, 0x8000000000008089ULL, 0x8000000000008003ULL,
        0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800AULL, 0x800000008000000AULL,
        0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
    static const int RHO[25] = {0,  1,  62, 28, 27, 36, 44, 6,  55, 20, 3,  10, 43,
                                25, 39, 41, 45, 15, 21, 8,  18, 2,  61, 56, 14};
    for (int round = 0; round < 24; round++) {
        uint64_t c[5], b[25];
        for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
        for (int x = 0; x < 5; x++) {
            const uint64_t d = c[(x + 4) % 5] ^ rotl64(c[(x + 1) % 5], 1);
            for (int y = 0; y < 25; y += 5) a[y + x] ^= d;
        }
        for (int x = 0; x < 5; x++)
            for (int y = 0; y < 5; y++) b[y + 5 * ((2 * x + 3 * y) % 5)] = rotl64(a[x + 5 * y], RHO[x + 5 * y]);
        for (int y = 0; y < 25; y += 5)
            for (int x = 0; x < 5; x++) a[y + x] = b[y + x] ^ (~b[y + (x + 1) % 5] & b[y + (x + 2) % 5]);
        a[0] ^= RC[round];
    }
}

inline uint64_t load_le64(const uint8_t* p) {
    uint64_t v = 0;
    for (int k = 7; k >= 0; k--) v = (v << 8) | p[k];
    return v;
}
inline void store_le64(uint8_t* p, uint64_t v) {
    for (int k = 0; k < 8; k++) p[k] = (uint8_t)(v >> (8 * k));
}

// out_len bytes of Keccak[capacity = 2 out_len](in); out_len is 32 or 64, `out` may alias `in`
inline void keccak(uint8_t* out, size_t out_len, const uint8_t* in, size_t len) {
    const size_t rate = 200 - 2 * out_len;
    uint64_t a[25] = {0};
    while (len >= rate) {
        for (size_t k = 0; k < rate / 8; k++) a[k] ^= load_le64(in + 8 * k);
        keccakf(a);
        in += rate;
        len -= rate;
    }
    uint8_t last[144] = {0};
    memcpy(last, in, len);
    last[len] ^= 0x01;
    last[rate - 1] ^= 0x80;
    for (size_t k = 0; k < rate / 8; k++) a[k] ^= load_le64(last + 8 * k);
    keccakf(a);
    for (size_t k = 0; k < out_len / 8; k++) store_le64(out + 8 * k, a[k]);
}
inline void keccak256(uint8_t out[32], const uint8_t* in, size_t len) { keccak(out, 32, in, len); }
inline void keccak512(uint8_t out[64], const uint8_t* in, size_t len) { keccak(out, 64, in, len); }

inline void seed_hash(uint64_t block, uint8_t out[32]) {
    memset(out, 0, 32);
    for (uint64_t i = 0; i < block / EPOCH_LENGTH; i++) keccak256(out, out, 32);
}

inline uint32_t load_le32(const uint8_t* p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// generateCache over `bytes` (a multiple of 64, at least 64, below 2^38) at `out`.  The bytes written are
// the reference's on a little-endian machine, which is also the layout the kernels read.
inline bool make_cache(const uint8_t seed[32], uint64_t bytes, uint8_t* out) {
    if (bytes < HASH_BYTES || bytes % HASH_BYTES != 0 || bytes / HASH_BYTES > 0xFFFFFFFFull) return false;
    const uint32_t rows = (uint32_t)(bytes / HASH_BYTES);
    const ModRecip rr = mod_recip(rows);
    keccak512(out, seed, 32);
    for (uint64_t r = 1; r < rows; r++) keccak512(out + r * HASH_BYTES, out + (r - 1) * HASH_BYTES, HASH_BYTES);
    uint8_t temp[HASH_BYTES];
    for (int round = 0; round < CACHE_ROUNDS; round++)
        for (uint64_t j = 0; j < rows; j++) {
            const uint8_t* src = out + ((j + rows - 1) % rows) * HASH_BYTES;
            uint8_t* dst = out + j * HASH_BYTES;
            const uint8_t* x = out + (uint64_t)mod_reduce(load_le32(dst), rr) * HASH_BYTES;
            for (size_t k = 0; k < HASH_BYTES; k++) temp[k] = src[k] ^ x[k];
            keccak512(dst, temp, HASH_BYTES);
        }
    return true;
}

// ---- the sealer's rounds (gsv_ethash_seal_batch).  A search launch cannot be interrupted, so a round is
// sized to SEAL_ROUND_ITEMS nonces, milliseconds of the full kernel, not to the caller's max_attempts:
// `headers` headers (a slice of those still searching) try `span` nonces each.  span is a multiple of the
// 256-lane workgroup unless the attempts left are fewer, never 0 while attempts are left, and headers * span
// <= SEAL_ROUND_ITEMS.
constexpr uint64_t SEAL_ROUND_ITEMS = 1ull << 22;
constexpr uint64_t SEAL_BLOCK = 256;

struct SealRound {
    uint64_t headers, span;
};

inline SealRound seal_round(uint64_t searching, uint64_t attempts_left) {
    if (searching == 0 || attempts_left == 0) return SealRound{0, 0};
    const uint64_t max_headers = SEAL_ROUND_ITEMS / SEAL_BLOCK;
    const uint64_t headers = searching < max_headers ? searching : max_headers;
    uint64_t span = SEAL_ROUND_ITEMS / headers / SEAL_BLOCK * SEAL_BLOCK;  // >= SEAL_BLOCK: headers <= max_headers
    if (span > attempts_left) span = attempts_left;
    return SealRound{headers, span};
}

}  // namespace ethash
}  // namespace gsv
