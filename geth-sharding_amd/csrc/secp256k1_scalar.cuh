// secp256k1 words and scalars for gfx950 — one item per lane.
//
// 256-bit values as 8 x 32-bit little-endian limbs held in VGPRs: the byte <-> limb conversions,
// the limb compares and the arithmetic mod the group order n (the moduli: secp256k1_dev.cuh).  Scalars are always
// FULLY reduced (< n) between operations, so equality / parity tests are plain limb compares.
// Products are 8x8 schoolbook product-scanning columns in inline asm (mul_asm.cuh); additions are
// __builtin_addc chains (v_add_co_u32 / v_addc_co_u32); reduction folds the high half with the
// 129-bit constant 2^256 - n.  The field mod p is secp256k1_fe9.cuh's (9 x 29-bit limbs); `fe` here
// is only the 8-word container a canonical field element travels in.
//
// This restates the MATH of libsecp256k1's scalar layer (scalar_8x32_impl.h in
// crypto/secp256k1/libsecp256k1/src) for a SIMD machine; the algorithms (limb width, reduction) are
// our own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GSV_DI __device__ __forceinline__

#include "mul_asm.cuh"
#include "opcount.cuh"
#include "secp256k1_dev.cuh"  // FP, SN, SNC, HALF_N

namespace gsv {

// a canonical field element (< p) as 8 words: what the kernels load, store and hash.  No arithmetic.
struct fe { uint32_t v[8]; };
struct sc { uint32_t v[8]; };

// ------------------------------------------------------------------ generic limb helpers
GSV_DI uint32_t lo32(uint64_t x) { return (uint32_t)x; }
GSV_DI uint32_t hi32(uint64_t x) { return (uint32_t)(x >> 32); }
// carry-chain primitives: lower to v_add_co_u32 / v_addc_co_u32 / v_sub(b)_co_u32 chains
GSV_DI uint32_t addc(uint32_t a, uint32_t b, uint32_t& c) {
    uint32_t co;
    uint32_t r = __builtin_addc(a, b, c, &co);
    c = co;
    return r;
}
GSV_DI uint32_t subb(uint32_t a, uint32_t b, uint32_t& br) {
    uint32_t bo;
    uint32_t r = __builtin_subc(a, b, br, &bo);
    br = bo;
    return r;
}

// big-endian 32 bytes <-> limbs
GSV_DI void limbs_from_be(uint32_t v[8], const uint8_t* b) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint8_t* p = b + 28 - 4 * i;
        v[i] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
    }
}
GSV_DI void load32_be(uint32_t v[8], const uint8_t* p) { limbs_from_be(v, p); }
GSV_DI void limbs_to_be(uint8_t* b, const uint32_t v[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint8_t* p = b + 28 - 4 * i;
        p[0] = (uint8_t)(v[i] >> 24);
        p[1] = (uint8_t)(v[i] >> 16);
        p[2] = (uint8_t)(v[i] >> 8);
        p[3] = (uint8_t)v[i];
    }
}

// a 32-bit word at any alignment (the 65-byte rows of signatures and keys)
GSV_DI uint32_t ld32u(const uint8_t* p) {
    uint32_t w;
    __builtin_memcpy(&w, p, 4);
    return w;
}
GSV_DI void st32u(uint8_t* p, uint32_t w) { __builtin_memcpy(p, &w, 4); }

GSV_DI bool limbs_zero(const uint32_t v[8]) {
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) o |= v[i];
    return o == 0;
}
// x < m ? (limb compare, m constant)
GSV_DI bool limbs_lt(const uint32_t x[8], const uint32_t m[8]) {
    uint32_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) (void)subb(x[i], m[i], br);
    return br != 0;
}

// ------------------------------------------------------------------ scalars mod n
// r = x mod n for x < 2^256 + small carry (at most one subtraction needed for x < 2n)
GSV_DI void sc_cond_sub_n(uint32_t r[8], const uint32_t x[8], uint32_t extra_carry) {
    uint32_t y[8], c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) y[i] = addc(x[i], i < 5 ? SNC[i] : 0u, c);
    uint32_t ge = c | extra_carry;
#pragma unroll
    for (int i = 0; i < 8; i++) r[i] = ge ? y[i] : x[i];
}

// 2^256 == SNC (mod n), SNC = SNC' + 2^128 with SNC' = SNC[0..3].  Reduce a 512-bit product
// by three folds hi * SNC -> lo (the hi part shrinks 256 -> 130 -> 35 -> 0 bits).
GSV_DI void sc_reduce(sc& r, const uint32_t t[16]) {
    const uint32_t C4[4] = {SNC[0], SNC[1], SNC[2], SNC[3]};
    // stage 1: m = L + H*SNC' + H*2^128  (< 2^386, 13 limbs)
    uint32_t p[12], m[13], c = 0;
    mul_8x4_fx(p, t + 8, C4);
#pragma unroll
    for (int i = 0; i < 8; i++) m[i] = addc(t[i], p[i], c);
#pragma unroll
    for (int i = 8; i < 12; i++) m[i] = addc(p[i], 0u, c);
    m[12] = c;
    c = 0;
#pragma unroll
    for (int i = 4; i < 12; i++) m[i] = addc(m[i], t[4 + i], c);
    m[12] += c;
    // stage 2: m2 = m[0..7] + m[8..12]*SNC' + m[8..12]*2^128  (< 2^291, 10 limbs)
    uint32_t p2[9], m2[10];
    mul_5x4_fx(p2, m + 8, C4);
    c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) m2[i] = addc(m[i], p2[i], c);
    m2[8] = addc(p2[8], 0u, c);
    m2[9] = c;
    c = 0;
#pragma unroll
    for (int i = 4; i < 9; i++) m2[i] = addc(m2[i], m[4 + i], c);
    m2[9] += c;
    // stage 3: m3 = m2[0..7] + m2[8..9]*SNC' + m2[8..9]*2^128  (< 2^256 + 2^166, carry limb 0/1)
    uint32_t p3[6], m3[8];
    mul_2x4_fx(p3, m2 + 8, C4);
    c = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) m3[i] = addc(m2[i], p3[i], c);
    m3[6] = addc(m2[6], 0u, c);
    m3[7] = addc(m2[7], 0u, c);
    uint32_t c2 = 0;
    m3[4] = addc(m3[4], m2[8], c2);
    m3[5] = addc(m3[5], m2[9], c2);
    m3[6] = addc(m3[6], 0u, c2);
    m3[7] = addc(m3[7], 0u, c2);
    // value = m3 + (c + c2) * 2^256 < 2^256 + 2^166 < 2n: one conditional subtraction
    sc_cond_sub_n(r.v, m3, c | c2);
}

GSV_DI void sc_mul(sc& r, const sc& a, const sc& b) {
    GSV_OPC(OPC_SC_MUL);
    uint32_t t[16];
    mul_8x8_fx(t, a.v, b.v);
    sc_reduce(r, t);
}
GSV_DI bool sc_is_zero(const sc& a) { return limbs_zero(a.v); }
GSV_DI void sc_neg(sc& r, const sc& a) {
    // n - a, 0 -> 0
    bool z = sc_is_zero(a);
    int64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        int64_t t = (int64_t)SN[i] - a.v[i] + br;
        r.v[i] = z ? 0u : (uint32_t)t;
        br = t >> 32;
    }
}
GSV_DI void sc_add(sc& r, const sc& a, const sc& b) {
    uint32_t s[8], c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = addc(a.v[i], b.v[i], c);
    sc_cond_sub_n(r.v, s, c);
}

GSV_DI void sc_from_const(sc& r, const uint32_t c[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = c[i];
}
GSV_DI bool sc_is_high(const sc& a) { return limbs_lt(HALF_N, a.v); }

// secp256k1_ec_seckey_verify, scalar_set_b32's overflow and scalar_is_zero: 0 < d < n
GSV_DI bool seckey_ok(const sc& d) { return limbs_lt(d.v, SN) && !sc_is_zero(d); }
// an invalid item runs the whole schedule on the scalar 1
GSV_DI void sc_set_one_unless(sc& k, bool ok) {
#pragma unroll
    for (int j = 0; j < 8; j++) k.v[j] = ok ? k.v[j] : (j == 0 ? 1u : 0u);
}

}  // namespace gsv
