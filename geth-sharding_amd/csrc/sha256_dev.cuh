// SHA-256's compression function (FIPS 180-4 6.2.2) on gfx950 VALU, one message per lane: the eight
// state words and a 16-word rolling schedule in registers.  The 64 rounds are unrolled in full, so
// every schedule index is a compile-time constant (a runtime index into a register array goes to
// scratch).  Rotations are v_alignbit_b32, Ch and Maj one v_bitop3_b32 each and the three-way XORs of
// the sigma functions another, as keccak_dev.cuh uses both.  Restates what libsecp256k1/src/
// hash_impl.h:13-127 computes (secp256k1_sha256_transform); words are big-endian words of the message.
// Free of HIP when compiled by a host compiler (tests/native/rfc6979_host.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SHA_FN __device__ __forceinline__
#define SHA_CONST __device__ constexpr
#else
#define SHA_FN static inline
#define SHA_CONST static constexpr
#endif

namespace gsv {

#include "sha256_consts.inc"

// v_bitop3_b32 truth tables (index = S0<<2 | S1<<1 | S2): Ch = S0 ? S1 : S2, Maj, S0^S1^S2
constexpr uint32_t SHA_BITOP3_CH = 0xCA;
constexpr uint32_t SHA_BITOP3_MAJ = 0xE8;
constexpr uint32_t SHA_BITOP3_XOR3 = 0x96;

#if defined(__HIPCC__)
template <int R>
SHA_FN uint32_t sha_rotr(uint32_t x) { return __builtin_amdgcn_alignbit(x, x, R); }
SHA_FN uint32_t sha_ch(uint32_t e, uint32_t f, uint32_t g) { return __builtin_amdgcn_bitop3_b32(e, f, g, SHA_BITOP3_CH); }
SHA_FN uint32_t sha_maj(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, SHA_BITOP3_MAJ); }
SHA_FN uint32_t sha_xor3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, SHA_BITOP3_XOR3); }
// (hi:lo) >> 8, low word: the byte shift of the 97-byte message's unaligned tail
SHA_FN uint32_t sha_align8(uint32_t hi, uint32_t lo) { return __builtin_amdgcn_alignbit(hi, lo, 8); }
#else
template <int R>
SHA_FN uint32_t sha_rotr(uint32_t x) { return (x >> R) | (x << (32 - R)); }
SHA_FN uint32_t sha_ch(uint32_t e, uint32_t f, uint32_t g) { return (e & f) | (~e & g); }
SHA_FN uint32_t sha_maj(uint32_t a, uint32_t b, uint32_t c) { return (a & b) | (a & c) | (b & c); }
SHA_FN uint32_t sha_xor3(uint32_t a, uint32_t b, uint32_t c) { return a ^ b ^ c; }
SHA_FN uint32_t sha_align8(uint32_t hi, uint32_t lo) { return (hi << 24) | (lo >> 8); }
#endif

SHA_FN uint32_t sha_Sig0(uint32_t x) { return sha_xor3(sha_rotr<2>(x), sha_rotr<13>(x), sha_rotr<22>(x)); }
SHA_FN uint32_t sha_Sig1(uint32_t x) { return sha_xor3(sha_rotr<6>(x), sha_rotr<11>(x), sha_rotr<25>(x)); }
SHA_FN uint32_t sha_sig0(uint32_t x) { return sha_xor3(sha_rotr<7>(x), sha_rotr<18>(x), x >> 3); }
SHA_FN uint32_t sha_sig1(uint32_t x) { return sha_xor3(sha_rotr<17>(x), sha_rotr<19>(x), x >> 10); }

// rounds I .. 63 over the rotating names (a .. h) and the schedule window w[i mod 16]
template <int I>
SHA_FN void sha256_rounds(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t e, uint32_t f, uint32_t g,
                          uint32_t h, uint32_t (&w)[16], uint32_t (&s)[8]) {
    if constexpr (I == 64) {
        s[0] += a; s[1] += b; s[2] += c; s[3] += d;
        s[4] += e; s[5] += f; s[6] += g; s[7] += h;
    } else {
        if constexpr (I >= 16)
            w[I & 15] += sha_sig0(w[(I + 1) & 15]) + w[(I + 9) & 15] + sha_sig1(w[(I + 14) & 15]);
        const uint32_t t1 = h + sha_Sig1(e) + sha_ch(e, f, g) + SHA256_K[I] + w[I & 15];
        const uint32_t t2 = sha_Sig0(a) + sha_maj(a, b, c);
        sha256_rounds<I + 1>(t1 + t2, a, b, c, d + t1, e, f, g, w, s);
    }
}

// s = compress(s, w); w is consumed (it ends as the last 16 schedule words)
SHA_FN void sha256_compress_inline(uint32_t (&s)[8], uint32_t (&w)[16]) {
    sha256_rounds<0>(s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], w, s);
}

#if defined(__HIPCC__)
// On the device the compression is ONE out-of-line function, called 16 times per nonce: inlined, the 16
// copies are ~190 KB of straight-line code (three times the instruction cache), and the round constants
// the compiler then keeps in scalar registers across them, with the values it spills for it, cost the
// signing kernel its second wave per SIMD.  State and block travel in VGPR vectors (an aggregate or
// pointer argument would pin them to scratch memory), as gej9_dbl_ool's point does (secp256k1_glv.cuh).
typedef uint32_t sha_v8 __attribute__((ext_vector_type(8)));
typedef uint32_t sha_v16 __attribute__((ext_vector_type(16)));
static __device__ __noinline__ sha_v8 sha256_compress_ool(sha_v8 sv, sha_v16 wv) {
    uint32_t s[8], w[16];
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = sv[i];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = wv[i];
    sha256_compress_inline(s, w);
    sha_v8 o;
#pragma unroll
    for (int i = 0; i < 8; i++) o[i] = s[i];
    return o;
}
// s = compress(s, w); w is left as it was
SHA_FN void sha256_compress(uint32_t (&s)[8], uint32_t (&w)[16]) {
    sha_v8 sv;
    sha_v16 wv;
#pragma unroll
    for (int i = 0; i < 8; i++) sv[i] = s[i];
#pragma unroll
    for (int i = 0; i < 16; i++) wv[i] = w[i];
    sv = sha256_compress_ool(sv, wv);
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = sv[i];
}
#else
SHA_FN void sha256_compress(uint32_t (&s)[8], uint32_t (&w)[16]) { sha256_compress_inline(s, w); }
#endif

SHA_FN void sha256_copy8(uint32_t (&o)[8], const uint32_t (&a)[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) o[i] = a[i];
}

}  // namespace gsv
