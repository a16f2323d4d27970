// Host build of csrc/sha256_dev.cuh and csrc/rfc6979_dev.cuh (their plain C++ forms), exported for
// tests/test_rfc6979_cpu.py.  Values cross the boundary as bytes; inside they are big-endian words in
// message order, as the device code holds them.
#include <cstddef>

#include "../../geth-sharding_amd/csrc/rfc6979_dev.cuh"
using namespace gsv;

static void ldw(uint32_t (&w)[8], const uint8_t* b) {
    for (int i = 0; i < 8; i++)
        w[i] = (uint32_t)b[4 * i] << 24 | (uint32_t)b[4 * i + 1] << 16 | (uint32_t)b[4 * i + 2] << 8 | b[4 * i + 3];
}
static void stw(uint8_t* b, const uint32_t (&w)[8]) {
    for (int i = 0; i < 8; i++)
        for (int j = 0; j < 4; j++) b[4 * i + j] = (uint8_t)(w[i] >> (24 - 8 * j));
}

extern "C" {
// SHA-256 of len bytes through sha256_compress alone: the padding is made here
void t_sha256(uint8_t* out32, const uint8_t* msg, size_t len) {
    uint32_t s[8];
    sha256_copy8(s, SHA256_IV);
    const size_t total = (len + 9 + 63) / 64 * 64;
    for (size_t off = 0; off < total; off += 64) {
        uint8_t blk[64];
        for (size_t i = 0; i < 64; i++) {
            size_t p = off + i;
            blk[i] = p < len ? msg[p] : p == len ? 0x80 : 0;
        }
        if (off + 64 == total)
            for (int i = 0; i < 8; i++) blk[56 + i] = (uint8_t)((uint64_t)len * 8 >> (56 - 8 * i));
        uint32_t w[16];
        for (int i = 0; i < 16; i++)
            w[i] = (uint32_t)blk[4 * i] << 24 | (uint32_t)blk[4 * i + 1] << 16 | (uint32_t)blk[4 * i + 2] << 8 |
                   blk[4 * i + 3];
        sha256_compress(s, w);
    }
    stw(out32, s);
}
// the two chaining values of a key (64 bytes: inner, outer); key == NULL: the all-zero key's constants
void t_hmac_mid(uint8_t* out64, const uint8_t* key32) {
    hmac_mid m;
    if (key32) {
        uint32_t k[8];
        ldw(k, key32);
        hmac_key(m, k);
    } else {
        hmac_key_zero(m);
    }
    stw(out64, m.in);
    stw(out64 + 32, m.out);
}
static void mid_of(hmac_mid& m, const uint8_t* key32) {
    uint32_t k[8];
    ldw(k, key32);
    hmac_key(m, k);
}
void t_hmac32(uint8_t* out32, const uint8_t* key32, const uint8_t* v32) {
    hmac_mid m;
    mid_of(m, key32);
    uint32_t v[8], o[8];
    ldw(v, v32);
    hmac32(o, m, v);
    stw(out32, o);
}
void t_hmac33(uint8_t* out32, const uint8_t* key32, const uint8_t* v32, int tag) {
    hmac_mid m;
    mid_of(m, key32);
    uint32_t v[8], o[8];
    ldw(v, v32);
    hmac33(o, m, v, (uint32_t)tag);
    stw(out32, o);
}
void t_hmac97(uint8_t* out32, const uint8_t* key32, const uint8_t* v32, int tag, const uint8_t* a32,
              const uint8_t* b32) {
    hmac_mid m;
    mid_of(m, key32);
    uint32_t v[8], a[8], b[8], o[8];
    ldw(v, v32);
    ldw(a, a32);
    ldw(b, b32);
    hmac97(o, m, v, (uint32_t)tag, a, b);
    stw(out32, o);
}
// n nonces: item i from key32[32 i], msg32[32 i]
void t_nonce(uint8_t* out32, const uint8_t* key32, const uint8_t* msg32, int n, unsigned counter) {
    for (int i = 0; i < n; i++) {
        uint32_t k[8], m[8], o[8];
        ldw(k, key32 + 32 * i);
        ldw(m, msg32 + 32 * i);
        rfc6979_nonce(o, k, m, counter);
        stw(out32 + 32 * i, o);
    }
}
}
