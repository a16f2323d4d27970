// RFC 6979's deterministic nonce as crypto.Sign gets it: libsecp256k1's nonce_function_rfc6979 with no
// extra data and no algorithm tag (libsecp256k1/src/secp256k1.c:310-340 over the HMAC-SHA256 generator
// of src/hash_impl.h:205-264), one item per lane.
//
//   V = 01 x 32, K = 00 x 32
//   K = HMAC(K, V || 00 || key || msg);  V = HMAC(K, V)
//   K = HMAC(K, V || 01 || key || msg);  V = HMAC(K, V)
//   output c: before every output after the first, K = HMAC(K, V || 00), V = HMAC(K, V);
//             then V = HMAC(K, V) is the output
//
// HMAC-SHA256 with a 32-byte key, at the three message lengths above (32, 33, 97 bytes), in fixed block
// shapes: no streaming state, no length argument.  A key's two padded blocks (key ^ ipad, key ^ opad)
// are compressed once per key (hmac_key) and the two chaining values serve every HMAC under that key;
// those of the all-zero first key are constants (sha256_consts.inc).  Compressions per nonce at
// counter 0: 3 (97 bytes under the constant key) + 2 + 2 (key 1: its blocks, V) + 3 (97 bytes)
// + 2 + 2 (key 2: its blocks, V) + 2 (the output) = 16; libsecp256k1, which compresses the key blocks
// again in every HMAC, spends 22.  Counter c costs 16 + 8 c.
//
// Values are eight big-endian words in message order: word j holds bytes 4j .. 4j + 3.  A 256-bit
// number in the field code's little-endian limbs v[8] is word j = v[7 - j], so no byte is swapped
// between the scalar code and this one.
#pragma once
#include "sha256_dev.cuh"

namespace gsv {

// a key's chaining values: SHA-256 state after key ^ 0x36.., and after key ^ 0x5c..
struct hmac_mid {
    uint32_t in[8], out[8];
};

SHA_FN void hmac_key(hmac_mid& m, const uint32_t (&key)[8]) {
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = key[i] ^ 0x36363636u;
#pragma unroll
    for (int i = 8; i < 16; i++) w[i] = 0x36363636u;
    sha256_copy8(m.in, SHA256_IV);
    sha256_compress(m.in, w);
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = key[i] ^ 0x5c5c5c5cu;
#pragma unroll
    for (int i = 8; i < 16; i++) w[i] = 0x5c5c5c5cu;
    sha256_copy8(m.out, SHA256_IV);
    sha256_compress(m.out, w);
}

SHA_FN void hmac_key_zero(hmac_mid& m) {
    sha256_copy8(m.in, HMAC0_IPAD);
    sha256_copy8(m.out, HMAC0_OPAD);
}

// the outer hash: the 32-byte inner digest after the opad block, 96 bytes in all
SHA_FN void hmac_outer(uint32_t (&o)[8], const hmac_mid& m, const uint32_t (&inner)[8]) {
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = inner[i];
    w[8] = 0x80000000u;
#pragma unroll
    for (int i = 9; i < 15; i++) w[i] = 0;
    w[15] = (64 + 32) * 8;
    sha256_copy8(o, m.out);
    sha256_compress(o, w);
}

// HMAC(key, v), 32 bytes: 2 compressions.  o may be v.
SHA_FN void hmac32(uint32_t (&o)[8], const hmac_mid& m, const uint32_t (&v)[8]) {
    uint32_t s[8];
    sha256_copy8(s, m.in);
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = v[i];
    w[8] = 0x80000000u;
#pragma unroll
    for (int i = 9; i < 15; i++) w[i] = 0;
    w[15] = (64 + 32) * 8;
    sha256_compress(s, w);
    hmac_outer(o, m, s);
}

// HMAC(key, v || tag), 33 bytes: 2 compressions
SHA_FN void hmac33(uint32_t (&o)[8], const hmac_mid& m, const uint32_t (&v)[8], uint32_t tag) {
    uint32_t s[8];
    sha256_copy8(s, m.in);
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = v[i];
    w[8] = (tag << 24) | 0x00800000u;
#pragma unroll
    for (int i = 9; i < 15; i++) w[i] = 0;
    w[15] = (64 + 33) * 8;
    sha256_compress(s, w);
    hmac_outer(o, m, s);
}

// HMAC(key, v || tag || a || b), 97 bytes: 3 compressions.  a and b sit one byte off the word grid.
SHA_FN void hmac97(uint32_t (&o)[8], const hmac_mid& m, const uint32_t (&v)[8], uint32_t tag,
                   const uint32_t (&a)[8], const uint32_t (&b)[8]) {
    uint32_t s[8];
    sha256_copy8(s, m.in);
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = v[i];
    w[8] = sha_align8(tag, a[0]);
#pragma unroll
    for (int i = 1; i < 8; i++) w[8 + i] = sha_align8(a[i - 1], a[i]);
    sha256_compress(s, w);
    w[0] = sha_align8(a[7], b[0]);
#pragma unroll
    for (int i = 1; i < 8; i++) w[i] = sha_align8(b[i - 1], b[i]);
    w[8] = sha_align8(b[7], 0x80000000u);
#pragma unroll
    for (int i = 9; i < 15; i++) w[i] = 0;
    w[15] = (64 + 97) * 8;
    sha256_compress(s, w);
    hmac_outer(o, m, s);
}

// the generator between two outputs: the current key's chaining values and V
struct rfc6979_gen {
    hmac_mid k;
    uint32_t v[8];
};

// RFC 6979 3.2 b-g (secp256k1_rfc6979_hmac_sha256_initialize over key || msg)
SHA_FN void rfc6979_init(rfc6979_gen& g, const uint32_t (&key)[8], const uint32_t (&msg)[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) g.v[i] = 0x01010101u;
    hmac_key_zero(g.k);
    // steps d-e and f-g differ in the tag byte alone: one copy of their seven compressions in the code
#pragma unroll 1
    for (uint32_t tag = 0; tag < 2; tag++) {
        uint32_t kk[8];
        hmac97(kk, g.k, g.v, tag, key, msg);
        hmac_key(g.k, kk);
        hmac32(g.v, g.k, g.v);
    }
}

// RFC 6979 3.2 h, the update between two outputs: K = HMAC(K, V || 00), V = HMAC(K, V)
SHA_FN void rfc6979_retry(rfc6979_gen& g) {
    uint32_t kk[8];
    hmac33(kk, g.k, g.v, 0x00u);
    hmac_key(g.k, kk);
    hmac32(g.v, g.k, g.v);
}

// nonce_function_rfc6979(out, msg, key, NULL, NULL, counter): a fresh generator's output number
// `counter`, as the reference makes it for every counter anew.  msg is the raw 32 bytes, not reduced
// mod n.  The signing kernel calls it once per counter too: no generator state stays in registers
// through the curve arithmetic, and a counter past 0 is never reached in practice.
SHA_FN void rfc6979_nonce(uint32_t (&out)[8], const uint32_t (&key)[8], const uint32_t (&msg)[8],
                          uint32_t counter) {
    rfc6979_gen g;
    rfc6979_init(g, key, msg);
#pragma unroll 1
    for (uint32_t c = 0;; c++) {
        hmac32(g.v, g.k, g.v);
        if (c == counter) break;
        rfc6979_retry(g);
    }
    sha256_copy8(out, g.v);
}

}  // namespace gsv
