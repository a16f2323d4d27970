// ECIES key derivation from an ECDH shared secret, for the curve's parameters ECIES_AES128_SHA256
// (crypto/ecies/params.go:69-76, 103) with the shared information s1 empty, which is what
// ecies.Encrypt(rand, pub, m, nil, nil) and the RLPx handshake use — one item per lane:
//
//   K  = SHA256(00 00 00 01 || X)     concatKDF (crypto/ecies/ecies.go:167-192) with kdLen = 32:
//                                     reps = ((32 + 7) * 8) / 512 = 0, one hash under counter 1
//   Ke = K[0:16]                      the AES-128 key
//   Km = SHA256(K[16:32])             the MAC key (ecies.go:273-277)
//
// Both messages (36 and 16 bytes) fit one padded block, so the derivation is two compressions in fixed
// block shapes: no streaming state, no length argument.  Values are big-endian words in message order,
// as in rfc6979_dev.cuh: the shared X as limbs v[8] is word j = v[7 - j].
// Free of HIP when compiled by a host compiler (tests/native/ecies_kdf_host.cpp).
#pragma once
#include "sha256_dev.cuh"

namespace gsv {

// x: the shared secret's 32 bytes as 8 words.  ke: Ke (16 bytes), km: Km (32 bytes).
SHA_FN void ecies_kdf_keys(uint32_t (&ke)[4], uint32_t (&km)[8], const uint32_t (&x)[8]) {
    uint32_t w[16], k[8];
    w[0] = 0x00000001u;  // the counter
#pragma unroll
    for (int i = 0; i < 8; i++) w[1 + i] = x[i];
    w[9] = 0x80000000u;
#pragma unroll
    for (int i = 10; i < 15; i++) w[i] = 0;
    w[15] = 36 * 8;
    sha256_copy8(k, SHA256_IV);
    sha256_compress(k, w);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        ke[i] = k[i];
        w[i] = k[4 + i];
    }
    w[4] = 0x80000000u;
#pragma unroll
    for (int i = 5; i < 15; i++) w[i] = 0;
    w[15] = 16 * 8;
    sha256_copy8(km, SHA256_IV);
    sha256_compress(km, w);
}

}  // namespace gsv
