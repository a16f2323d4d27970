// RIPEMD-160's compression function on gfx950 VALU, one message per lane: the five state words and the
// 16 little-endian message words in registers.  The two lines of 80 steps are unrolled in full, so every
// word index and rotate amount is a compile-time constant (a runtime index into a register array goes
// to scratch).  Each of the five round functions is one v_bitop3_b32, each rotation one v_alignbit_b32.
// Step j of the left line is followed by step j of the right line: the two chains share only the
// message words, so one's adds and rotates fill the other's dependency stalls.
// Restates what vendor/golang.org/x/crypto/ripemd160/ripemd160block.go computes (_Block), from the
// algorithm's specification.  Free of HIP when compiled by a host compiler (tests/native/md_hash_host.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RMD_FN __device__ __forceinline__
#define RMD_CONST __device__ constexpr
#else
#define RMD_FN static inline
#define RMD_CONST static constexpr
#endif

namespace gsv {

#include "ripemd160_consts.inc"

// The round functions by number: x^y^z, (x&y)|(~x&z), (x|~y)^z, (x&z)|(y&~z), x^(y|~z)
template <int F>
constexpr uint32_t rmd_f_plain(uint32_t x, uint32_t y, uint32_t z) {
    return F == 0 ? x ^ y ^ z : F == 1 ? (x & y) | (~x & z) : F == 2 ? (x | ~y) ^ z : F == 3 ? (x & z) | (y & ~z) : x ^ (y | ~z);
}
// v_bitop3_b32 truth tables (index = S0<<2 | S1<<1 | S2): the function of the three index bits' columns
template <int F>
constexpr uint32_t RMD_BITOP3 = rmd_f_plain<F>(0xF0u, 0xCCu, 0xAAu) & 0xFFu;
static_assert(RMD_BITOP3<0> == 0x96 && RMD_BITOP3<1> == 0xCA && RMD_BITOP3<2> == 0x59 && RMD_BITOP3<3> == 0xE4 &&
                  RMD_BITOP3<4> == 0x2D,
              "round function truth tables");

#if defined(__HIPCC__)
template <int F>
RMD_FN uint32_t rmd_f(uint32_t x, uint32_t y, uint32_t z) { return __builtin_amdgcn_bitop3_b32(x, y, z, RMD_BITOP3<F>); }
template <int S>
RMD_FN uint32_t rmd_rol(uint32_t x) { return __builtin_amdgcn_alignbit(x, x, 32 - S); }
#else
template <int F>
RMD_FN uint32_t rmd_f(uint32_t x, uint32_t y, uint32_t z) { return rmd_f_plain<F>(x, y, z); }
template <int S>
RMD_FN uint32_t rmd_rol(uint32_t x) { return (x << S) | (x >> (32 - S)); }
#endif

// steps J .. 79 of both lines over the rotating names: a step computes
// T = rol(A + f(B, C, D) + X[r] + K, s) + E and renames (A, B, C, D, E) <- (E, T, B, rol(C, 10), D)
template <int J>
RMD_FN void rmd_steps(uint32_t al, uint32_t bl, uint32_t cl, uint32_t dl, uint32_t el, uint32_t ar, uint32_t br,
                      uint32_t cr, uint32_t dr, uint32_t er, const uint32_t (&x)[16], uint32_t (&h)[5]) {
    if constexpr (J == 80) {
        const uint32_t t = h[1] + cl + dr;
        h[1] = h[2] + dl + er;
        h[2] = h[3] + el + ar;
        h[3] = h[4] + al + br;
        h[4] = h[0] + bl + cr;
        h[0] = t;
    } else {
        constexpr int R = J / 16;
        const uint32_t tl = rmd_rol<RMD_SL[J]>(al + rmd_f<R>(bl, cl, dl) + x[RMD_RL[J]] + RMD_KL[R]) + el;
        const uint32_t tr = rmd_rol<RMD_SR[J]>(ar + rmd_f<4 - R>(br, cr, dr) + x[RMD_RR[J]] + RMD_KR[R]) + er;
        rmd_steps<J + 1>(el, tl, bl, rmd_rol<10>(cl), dl, er, tr, br, rmd_rol<10>(cr), dr, x, h);
    }
}

// h = compress(h, x); x is 16 little-endian words of the block
RMD_FN void ripemd160_compress(uint32_t (&h)[5], const uint32_t (&x)[16]) {
    rmd_steps<0>(h[0], h[1], h[2], h[3], h[4], h[0], h[1], h[2], h[3], h[4], x, h);
}

RMD_FN void ripemd160_init(uint32_t (&h)[5]) {
#pragma unroll
    for (int i = 0; i < 5; i++) h[i] = RMD_IV[i];
}

}  // namespace gsv
