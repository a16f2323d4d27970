// AES-128 encryption (FIPS-197) for one block per lane on gfx950: the cipher of ECIES_AES128_SHA256's CTR
// keystream (crypto/ecies/params.go:69-76).  The 44 round-key words live in registers (every index is a
// compile-time constant: a runtime index into a register array goes to scratch); rounds 1-9 read ONE
// 1 KiB table of SubBytes + MixColumns columns, Te0[x] = {02 s, s, s, 03 s} with s = S[x], and take the
// other three columns as rotations of it (v_alignbit_b32).  The S-box itself is byte 1 of Te0, so the
// last round and the key schedule read the same table: one table, 1 KiB of LDS per workgroup
// (aes_te0_fill).  Words are big-endian words of the block, as sha256_dev.cuh's are of the message.
// Table lookups are indexed by key-dependent bytes: not hardened against a co-tenant (include/gsv.h).
// Free of HIP when compiled by a host compiler (tests/native/ecies_sym_host.cpp).
#pragma once
#include <stdint.h>

#include "sha256_dev.cuh"  // SHA_FN / SHA_CONST, sha_rotr

namespace gsv {

// FIPS-197 figure 7
SHA_CONST uint8_t AES_SBOX[256] = {
    0x63, 0x7c, 0x77, 0x7b, 0xf2, 0x6b, 0x6f, 0xc5, 0x30, 0x01, 0x67, 0x2b, 0xfe, 0xd7, 0xab, 0x76,
    0xca, 0x82, 0xc9, 0x7d, 0xfa, 0x59, 0x47, 0xf0, 0xad, 0xd4, 0xa2, 0xaf, 0x9c, 0xa4, 0x72, 0xc0,
    0xb7, 0xfd, 0x93, 0x26, 0x36, 0x3f, 0xf7, 0xcc, 0x34, 0xa5, 0xe5, 0xf1, 0x71, 0xd8, 0x31, 0x15,
    0x04, 0xc7, 0x23, 0xc3, 0x18, 0x96, 0x05, 0x9a, 0x07, 0x12, 0x80, 0xe2, 0xeb, 0x27, 0xb2, 0x75,
    0x09, 0x83, 0x2c, 0x1a, 0x1b, 0x6e, 0x5a, 0xa0, 0x52, 0x3b, 0xd6, 0xb3, 0x29, 0xe3, 0x2f, 0x84,
    0x53, 0xd1, 0x00, 0xed, 0x20, 0xfc, 0xb1, 0x5b, 0x6a, 0xcb, 0xbe, 0x39, 0x4a, 0x4c, 0x58, 0xcf,
    0xd0, 0xef, 0xaa, 0xfb, 0x43, 0x4d, 0x33, 0x85, 0x45, 0xf9, 0x02, 0x7f, 0x50, 0x3c, 0x9f, 0xa8,
    0x51, 0xa3, 0x40, 0x8f, 0x92, 0x9d, 0x38, 0xf5, 0xbc, 0xb6, 0xda, 0x21, 0x10, 0xff, 0xf3, 0xd2,
    0xcd, 0x0c, 0x13, 0xec, 0x5f, 0x97, 0x44, 0x17, 0xc4, 0xa7, 0x7e, 0x3d, 0x64, 0x5d, 0x19, 0x73,
    0x60, 0x81, 0x4f, 0xdc, 0x22, 0x2a, 0x90, 0x88, 0x46, 0xee, 0xb8, 0x14, 0xde, 0x5e, 0x0b, 0xdb,
    0xe0, 0x32, 0x3a, 0x0a, 0x49, 0x06, 0x24, 0x5c, 0xc2, 0xd3, 0xac, 0x62, 0x91, 0x95, 0xe4, 0x79,
    0xe7, 0xc8, 0x37, 0x6d, 0x8d, 0xd5, 0x4e, 0xa9, 0x6c, 0x56, 0xf4, 0xea, 0x65, 0x7a, 0xae, 0x08,
    0xba, 0x78, 0x25, 0x2e, 0x1c, 0xa6, 0xb4, 0xc6, 0xe8, 0xdd, 0x74, 0x1f, 0x4b, 0xbd, 0x8b, 0x8a,
    0x70, 0x3e, 0xb5, 0x66, 0x48, 0x03, 0xf6, 0x0e, 0x61, 0x35, 0x57, 0xb9, 0x86, 0xc1, 0x1d, 0x9e,
    0xe1, 0xf8, 0x98, 0x11, 0x69, 0xd9, 0x8e, 0x94, 0x9b, 0x1e, 0x87, 0xe9, 0xce, 0x55, 0x28, 0xdf,
    0x8c, 0xa1, 0x89, 0x0d, 0xbf, 0xe6, 0x42, 0x68, 0x41, 0x99, 0x2d, 0x0f, 0xb0, 0x54, 0xbb, 0x16};

// Measured and not kept: the three rotations as tables of their own (4 KiB of LDS, no v_alignbit_b32 in
// the rounds) ran the symmetric kernels in the same time (profiles/ecies/ab_tables.json).
constexpr int AES_TE0_WORDS = 256;

// Te0[x]: the column MixColumns makes of S[x] in row 0, as a big-endian word {02 s, s, s, 03 s}
SHA_FN uint32_t aes_te0_entry(uint32_t x) {
    const uint32_t s = AES_SBOX[x];
    const uint32_t s2 = ((s << 1) ^ ((s >> 7) * 0x11Bu)) & 0xFFu;  // xtime (4.2.1)
    return (s2 << 24) | (s << 16) | (s << 8) | (s2 ^ s);
}

// te[AES_TE0_WORDS] (LDS on the device): entry t by thread t of the first 256; the caller synchronises afterwards
SHA_FN void aes_te0_fill(uint32_t* te, uint32_t t) {
    if (t < (uint32_t)AES_TE0_WORDS) te[t] = aes_te0_entry(t);
}

SHA_FN uint32_t aes_sub(const uint32_t* te, uint32_t x) { return (te[x] >> 8) & 0xFFu; }

// SubWord(RotWord(w)) (5.2): the bytes of w rotated left by one, each through the S-box
SHA_FN uint32_t aes_sub_rot_word(const uint32_t* te, uint32_t w) {
    return (aes_sub(te, (w >> 16) & 0xFFu) << 24) | (aes_sub(te, (w >> 8) & 0xFFu) << 16) |
           (aes_sub(te, w & 0xFFu) << 8) | aes_sub(te, w >> 24);
}

// KeyExpansion (5.2): rk[0..3] = the key's big-endian words
SHA_FN void aes128_expand(uint32_t (&rk)[44], const uint32_t (&key)[4], const uint32_t* te) {
#pragma unroll
    for (int i = 0; i < 4; i++) rk[i] = key[i];
    uint32_t rcon = 0x01000000u;
#pragma unroll
    for (int r = 1; r <= 10; r++) {
        rk[4 * r] = rk[4 * r - 4] ^ aes_sub_rot_word(te, rk[4 * r - 1]) ^ rcon;
        rk[4 * r + 1] = rk[4 * r - 3] ^ rk[4 * r];
        rk[4 * r + 2] = rk[4 * r - 2] ^ rk[4 * r + 1];
        rk[4 * r + 3] = rk[4 * r - 1] ^ rk[4 * r + 2];
        rcon = r == 8 ? 0x1B000000u : rcon << 1;
    }
}

// one column of a round: SubBytes, ShiftRows and MixColumns of the bytes (a0 row 0, a1 row 1, ...)
SHA_FN uint32_t aes_col(const uint32_t* te, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3) {
    return te[a0 >> 24] ^ sha_rotr<8>(te[(a1 >> 16) & 0xFFu]) ^ sha_rotr<16>(te[(a2 >> 8) & 0xFFu]) ^
           sha_rotr<24>(te[a3 & 0xFFu]);
}
SHA_FN uint32_t aes_last(const uint32_t* te, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3) {
    return (aes_sub(te, a0 >> 24) << 24) | (aes_sub(te, (a1 >> 16) & 0xFFu) << 16) |
           (aes_sub(te, (a2 >> 8) & 0xFFu) << 8) | aes_sub(te, a3 & 0xFFu);
}

// Cipher (5.1): out = AES-128(in), both as big-endian words
SHA_FN void aes128_encrypt(uint32_t (&out)[4], const uint32_t (&in)[4], const uint32_t (&rk)[44],
                           const uint32_t* te) {
    uint32_t s0 = in[0] ^ rk[0], s1 = in[1] ^ rk[1], s2 = in[2] ^ rk[2], s3 = in[3] ^ rk[3];
#pragma unroll
    for (int r = 1; r < 10; r++) {
        const uint32_t t0 = aes_col(te, s0, s1, s2, s3) ^ rk[4 * r];
        const uint32_t t1 = aes_col(te, s1, s2, s3, s0) ^ rk[4 * r + 1];
        const uint32_t t2 = aes_col(te, s2, s3, s0, s1) ^ rk[4 * r + 2];
        const uint32_t t3 = aes_col(te, s3, s0, s1, s2) ^ rk[4 * r + 3];
        s0 = t0, s1 = t1, s2 = t2, s3 = t3;
    }
    out[0] = aes_last(te, s0, s1, s2, s3) ^ rk[40];
    out[1] = aes_last(te, s1, s2, s3, s0) ^ rk[41];
    out[2] = aes_last(te, s2, s3, s0, s1) ^ rk[42];
    out[3] = aes_last(te, s3, s0, s1, s2) ^ rk[43];
}

// the CTR counter of Go's cipher.NewCTR: the whole block one big-endian integer, + 1 with carry through
// all 128 bits
SHA_FN void aes_ctr_inc(uint32_t (&c)[4]) {
    c[3] += 1u;
    uint32_t carry = c[3] == 0u;
    c[2] += carry;
    carry = carry & (c[2] == 0u);
    c[1] += carry;
    carry = carry & (c[1] == 0u);
    c[0] += carry;
}

}  // namespace gsv
