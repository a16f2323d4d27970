// The message half of ecies.Encrypt / Decrypt for ECIES_AES128_SHA256 (crypto/ecies/ecies.go:196-292,
// 358-365), one item per lane: a streaming HMAC-SHA256 (sha256_dev.cuh's out-of-line compression) fused
// with the AES-128-CTR keystream (aes128_dev.cuh).
//
//   tag = HMAC-SHA256(Km, em || s2),  em = iv || C,  C = data XOR CTR(Ke, iv)
//
// The inner hash runs over  ipad block | em | s2 | padding.  em starts on a block boundary, so a 64-byte
// SHA-256 block holds four 16-byte groups of em that are AES blocks of C (the first group of the first
// block is the IV): every data dword is loaded once, XORed with the keystream, hashed (as ciphertext,
// whichever direction) and stored.  Decrypt writes the plaintext BEFORE the tag is known; the caller
// zeroes it again when the tag does not match (ecies.hip).  The boundary between em and s2 falls at any
// byte of a block; both are read from any byte offset as aligned dwords, realigned as keccak.hip's
// load_block does it, and no dword is read that does not hold a valid byte.  Words are big-endian words
// of the stream.  Every index into a register array is a compile-time constant.
// Free of HIP when compiled by a host compiler (tests/native/ecies_sym_host.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "aes128_dev.cuh"

namespace gsv {

#if defined(__HIPCC__)
SHA_FN uint32_t sym_ld32(uintptr_t q) { return *(const uint32_t*)q; }
// (hi:lo) >> 8 sh, low word
SHA_FN uint32_t sym_alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) { return __builtin_amdgcn_alignbyte(hi, lo, sh); }
#else
SHA_FN uint32_t sym_ld32(uintptr_t q) {
    uint32_t v;
    __builtin_memcpy(&v, (const void*)q, 4);
    return v;
}
SHA_FN uint32_t sym_alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) {
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh));
}
#endif

// the bytes of the big-endian word at block positions pos .. pos + 3 that lie in [lo, hi)
SHA_FN uint32_t sym_mask(int32_t pos, int32_t lo, int32_t hi) {
    const int32_t a = lo - pos, b = hi - pos;
    const uint32_t m_lo = a <= 0 ? 0xFFFFFFFFu : a >= 4 ? 0u : 0xFFFFFFFFu >> (8 * a);
    const uint32_t m_hi = b >= 4 ? 0xFFFFFFFFu : b <= 0 ? 0u : ~(0xFFFFFFFFu >> (8 * b));
    return m_lo & m_hi;
}

// w |= the bytes at block positions [lo, hi) (0 <= lo < hi <= 64) of the string whose byte for block
// position t is at address v + t; v has any alignment.  Up to 17 aligned dwords from v rounded down to
// 4; a dword is read only if it holds a byte of [lo, hi).
SHA_FN void sym_load_be(uint32_t (&w)[16], uintptr_t v, int32_t lo, int32_t hi) {
    const uint32_t sh = (uint32_t)(v & 3u);
    const uintptr_t q = v - sh;
    uint32_t d[17];
#pragma unroll
    for (int j = 0; j < 17; j++) {
        const int32_t first = 4 * j - (int32_t)sh;  // block position of the dword's first byte
        d[j] = (first + 3 >= lo && first < hi) ? sym_ld32(q + 4u * j) : 0u;
    }
#pragma unroll
    for (int j = 0; j < 16; j++)
        w[j] |= __builtin_bswap32(sym_alignbyte(d[j + 1], d[j], sh)) & sym_mask(4 * j, lo, hi);
}

// the chaining value after the key block of HMAC-SHA256: SHA256 over (Km || zeros) ^ pad
SHA_FN void hmac_key_state(uint32_t (&s)[8], const uint32_t (&km)[8], uint32_t pad) {
    uint32_t w[16];
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = (j < 8 ? km[j] : 0u) ^ pad;
    sha256_copy8(s, SHA256_IV);
    sha256_compress(s, w);
}

// ENC: `in` = the message, `out` = C.  !ENC: `in` = C, `out` = the message.  Both dlen bytes at any
// alignment (out is written byte by byte, and only its dlen bytes).  iv: the counter block's four
// words.  s2: s2len bytes at any alignment (not read when s2len == 0).  te: aes_te0_fill's table.
// tag: HMAC-SHA256(Km, iv || C || s2).  dlen, s2len < 2^32.
template <bool ENC>
SHA_FN void ecies_sym(uint32_t (&tag)[8], const uint32_t (&ke)[4], const uint32_t (&km)[8], const uint8_t* in,
                      uint32_t dlen, const uint32_t (&iv)[4], const uint8_t* s2, uint32_t s2len, uint8_t* out,
                      const uint32_t* te) {
    uint32_t rk[44], ctr[4], s[8];
    aes128_expand(rk, ke, te);
#pragma unroll
    for (int i = 0; i < 4; i++) ctr[i] = iv[i];
    hmac_key_state(s, km, 0x36363636u);
    const uint64_t emlen = 16ull + dlen, total = emlen + s2len;  // em, em || s2
    const uint64_t nblocks = (total + 72) / 64;                  // 0x80, zeros, the 64-bit length
    for (uint64_t blk = 0, o = 0; blk < nblocks; blk++, o += 64) {
        uint32_t w[16];
#pragma unroll
        for (int j = 0; j < 16; j++) w[j] = 0u;
        const int32_t d_lo = o == 0 ? 16 : 0;
        const int32_t d_hi = o >= emlen ? 0 : emlen - o >= 64 ? 64 : (int32_t)(emlen - o);
        if (o == 0) {
#pragma unroll
            for (int i = 0; i < 4; i++) w[i] = iv[i];
        }
        if (d_hi > d_lo) {
            sym_load_be(w, (uintptr_t)in + (uintptr_t)o - 16u, d_lo, d_hi);
#pragma unroll
            for (int g = 0; g < 4; g++) {
                if (16 * g >= d_lo && 16 * g < d_hi) {
                    uint32_t ks[4];
                    aes128_encrypt(ks, ctr, rk, te);
                    aes_ctr_inc(ctr);
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int32_t pos = 16 * g + 4 * i;
                        const uint32_t x = (w[4 * g + i] ^ ks[i]) & sym_mask(pos, d_lo, d_hi);
                        if (ENC) w[4 * g + i] = x;
                        uint8_t* p = out + (size_t)(o + (uint64_t)pos - 16u);
#pragma unroll
                        for (int b = 0; b < 4; b++)
                            if (pos + b < d_hi) p[b] = (uint8_t)(x >> (24 - 8 * b));
                    }
                }
            }
        }
        // s2 from block position emlen - o on
        const int32_t s_lo = o >= emlen ? 0 : d_hi;
        const int32_t s_hi = o >= total ? 0 : total - o >= 64 ? 64 : (int32_t)(total - o);
        if (s_lo < 64 && s_hi > s_lo) sym_load_be(w, (uintptr_t)s2 + (uintptr_t)o - (uintptr_t)emlen, s_lo, s_hi);
        // padding: 0x80 behind the last byte, the length in bits (ipad block included) in the last block
        if (total >= o && total - o < 64) {
            const uint32_t p = (uint32_t)(total - o);
#pragma unroll
            for (int j = 0; j < 16; j++)
                if ((uint32_t)j == (p >> 2)) w[j] |= 0x80000000u >> (8 * (p & 3u));
        }
        if (blk + 1 == nblocks) {
            const uint64_t bits = (64 + total) * 8;
            w[14] |= (uint32_t)(bits >> 32);
            w[15] |= (uint32_t)bits;
        }
        sha256_compress(s, w);
    }
    // outer hash: opad block, the inner digest, padding
    uint32_t w[16];
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = s[j];
    w[8] = 0x80000000u;
#pragma unroll
    for (int j = 9; j < 15; j++) w[j] = 0u;
    w[15] = (64 + 32) * 8;
    hmac_key_state(tag, km, 0x5c5c5c5cu);
    sha256_compress(tag, w);
}

}  // namespace gsv
