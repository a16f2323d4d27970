// The integer-only pieces of the secp256k1 recovery's scalar schedule (secp256k1_glv.cuh binds them to
// its constants): the GLV ladder's digits read from the scalar's bits, and the split's two short
// products.  Plain C++ when __HIPCC__ is not defined, so tests/native/recover_trim_host.cpp runs the
// same text on the CPU (there the 4 x 4 product is a loop instead of mul_asm.cuh's statement).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "mul_asm.cuh"  // mul_4x4_fx
#define GLV_FN __device__ __forceinline__
#else
#define GLV_FN static inline
#endif

namespace gsv {

// Fixed-schedule odd-digit recoding, window w, T + 1 digits: an odd k < 2^(w (T + 1)) is
// sum d_i 2^(w i) with d_i odd in [-(2^w - 1), 2^w - 1], and the digits are read straight from k's
// bits.  With K = k >> 1 and K_i = (K >> w i) & (2^w - 1):  d_i = 2 K_i - (2^w - 1) for i < T and the
// top digit is d_T = 2 (K >> w T) + 1, because sum_{i < T} (2 K_i - (2^w - 1)) 2^(w i) =
// 2 (K mod 2^(w T)) - (2^(w T) - 1), and d_T 2^(w T) makes up the rest: 2 K + 1 = k.  (The
// subtract-and-shift loop this replaced gave the same digits: tests/test_secp_recover_trim.py holds
// it against tests/secp_glv_model.py's recode.)
// The code the ladder consumes is a sign above a (w - 1)-bit table index (|d| - 1) / 2:
// K_i >= 2^(w-1) is d > 0 with index K_i - 2^(w-1); below, d < 0 with index 2^(w-1) - 1 - K_i, the low
// bits of K_i complemented.  The top digit is positive and its index is K >> w T itself.

// K = k >> 1 in NW words (k has NW + 1 words or more)
template <int NW>
GLV_FN void glv_halve(uint32_t (&K)[NW], const uint32_t* k) {
#pragma unroll
    for (int i = 0; i < NW; i++) K[i] = (k[i] >> 1) | (k[i + 1] << 31);
}
// The ladder takes the digits from the top, and T is a multiple of the slots per word: the top digit
// is the low slot of K[NW - 1], and K[NW - 2] is the word of the digits being consumed.  When its
// lowest slot is used up, glv_next_word moves the words below it up by one: plain register moves,
// where a word picked by the loop counter becomes a scratch array read by a dynamic offset.
// digit i's slot in the word that holds it (32 % w == 0: a slot never straddles two words)
template <int W>
GLV_FN uint32_t glv_slot(uint32_t word, int i) {
    static_assert(32 % W == 0, "a slot never straddles two words");
    return (word >> (((uint32_t)i % (32 / W)) * W)) & ((1u << W) - 1u);
}
template <int NW>
GLV_FN void glv_next_word(uint32_t (&K)[NW]) {
#pragma unroll
    for (int k = NW - 2; k > 0; k--) K[k] = K[k - 1];
}
// digit i < T from K_i: the table index and whether the digit is negative
template <int W>
GLV_FN void glv_digit(uint32_t& idx, bool& neg, uint32_t slot) {
    constexpr uint32_t HALF = 1u << (W - 1);
    neg = (slot & HALF) == 0;
    idx = (slot ^ (neg ? HALF - 1u : 0u)) & (HALF - 1u);
}

// t[0..7] = a[0..3] * b[0..3]
GLV_FN void glv_mul_4x4(uint32_t t[8], const uint32_t a[4], const uint32_t b[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
    mul_4x4_fx(t, a, b);
#else
    for (int i = 0; i < 8; i++) t[i] = 0;
    for (int i = 0; i < 4; i++) {
        uint64_t c = 0;
        for (int j = 0; j < 4; j++) {
            c += (uint64_t)a[i] * b[j] + t[i + j];  // < 2^64: (2^32 - 1)^2 + 2 (2^32 - 1)
            t[i + j] = (uint32_t)c;
            c >>= 32;
        }
        t[i + 4] = (uint32_t)c;
    }
#endif
}

// r2 = c1 nb1 - c2 b2 (mod n) for c1, c2, nb1, b2 < 2^128 with c1 nb1 < n and c2 b2 < n (the caller
// says why): two 4 x 4-limb products, one subtraction, n added back when it borrows.  No 512-bit
// product and no reduction.
GLV_FN void glv_short_r2(uint32_t r2[8], const uint32_t c1[4], const uint32_t nb1[4], const uint32_t c2[4],
                         const uint32_t b2[4], const uint32_t n[8]) {
    uint32_t p1[8], p2[8];
    glv_mul_4x4(p1, c1, nb1);
    glv_mul_4x4(p2, c2, b2);
    uint32_t d[8];
    int64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        int64_t t = (int64_t)p1[i] - p2[i] + br;
        d[i] = (uint32_t)t;
        br = t >> 32;
    }
    const bool neg = br != 0;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c += (uint64_t)d[i] + (neg ? n[i] : 0u);
        r2[i] = (uint32_t)c;
        c >>= 32;
    }
}

}  // namespace gsv
