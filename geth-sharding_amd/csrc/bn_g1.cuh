// BN254 G1 for the bn256Add (0x06) and bn256ScalarMul (0x07) precompiles (core/vm/contracts.go:274-312;
// G1.Add / G1.ScalarMult / G1.Unmarshal / G1.Marshal, crypto/bn256/cloudflare/bn256.go:62-78, 98-158).
// One item per lane; everything here also compiles for the host (plain C++ when __HIPCC__ is not
// defined), where tests/native/bn_g1_recode_host.cpp runs the recoding and the whole item functions.
//
// Scalar multiplication.  The reference (curve.go:185-207, lattice.go) splits k with the curve's
// endomorphism phi(x, y) = (beta x, y) = lambda (x, y); so does the fast path here:
//   g1_glv_split    k = k1 + k2 lambda (mod r) for any k < 2^256 (no reduction mod r first), k1 and k2
//                   signed with |k1|, |k2| < 2^127 (one rounded product each with the lattice's
//                   precomputed reciprocals); the signs move onto the points
//   table           T1 = +-P, T2 = +-phi(P), T3 = T1 + T2 without an inversion: T3 = (X3, Y3, Z3) is
//                   computed Jacobian, and T1, T2 are rescaled to that Z3.  With a common Z the three
//                   (X, Y) are AFFINE points of the isomorphic curve y^2 = x^3 + 3 Z3^6 (the doubling
//                   and addition formulas do not contain the constant term), the loop runs there with
//                   mixed additions, and Z3 is multiplied into the result's Z before the one inversion
//   loop            128 joint bits: a doubling (7 products) and, for a nonzero bit pair, one mixed
//                   addition of the selected entry (11 products)
// The bit-serial form (256 doublings, a mixed addition of P per set bit) is the same code without
// the split: the A/B partner and second implementation (launcher argument).
// The additions are complete (infinity, equal operands -> doubling, opposite operands -> infinity), as
// the reference's are (curve.go:65-120): a joint-bit accumulator can meet +-(table entry) when
// k1 + k2 lambda is a multiple of r.
#pragma once
#include "bn254_fe9.cuh"

namespace gsv {
namespace bn {

// p as eight little-endian 32-bit words (constants.go:31 P)
FQ_DEVCONST uint32_t BN_P_W[8] = {0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u,
                                  0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};

// gfP.Unmarshal (gfp.go:61-78) + montEncode: big-endian bytes -> Montgomery form (R = 2^261);
// false if the coordinate is >= p
FQ_FN bool fp_unmarshal(fq& r, const uint8_t* p) {
    uint32_t x[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint8_t* q = p + 28 - 4 * i;
        x[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
    }
    int64_t br = 0;  // x - p: the final borrow says x < p
#pragma unroll
    for (int i = 0; i < 8; i++) br = ((int64_t)x[i] - (int64_t)BN_P_W[i] + br) >> 32;
    bool ok = br != 0;
#pragma unroll
    for (int i = 0; i < 8; i++) x[i] = ok ? x[i] : 0u;
    r = fq_store(fq_mul(fq_from_words(x), fq_const(FQ_R2)));
    return ok;
}
// montDecode + big-endian marshal (gfp.go:51-59): the canonical residue of a R^-1
FQ_FN void fp_marshal(uint8_t* out, const fq& a) {
    fqm<1, 1> one{{1, 0, 0, 0, 0, 0, 0, 0, 0}};
    uint32_t w[8];
    fq_to_words(w, fq_canon(fq_mul(a, one)));
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint32_t x = w[7 - i];
        out[4 * i] = (uint8_t)(x >> 24);
        out[4 * i + 1] = (uint8_t)(x >> 16);
        out[4 * i + 2] = (uint8_t)(x >> 8);
        out[4 * i + 3] = (uint8_t)x;
    }
}

// ---------------------------------------------------------------------------- scalar recoding
// The lattice {(a, b): a + b lambda = 0 (mod r)} of lambda = 0x30644e72e131a029048b6e193fd84104
// cc37a73fec2bc5e9b8ca0b2d36636f23 (phi(P) = lambda P for beta = FQ_XI_PSQ1_3, the reference's
// xiTo2PSquaredMinus2Over3, curve.go:189) has the reduced basis
//   v1 = (147946756881789319000765030803803410728, -9931322734385697763)
//   v2 = (9931322734385697763, 147946756881789319010696353538189108491),   det = r.
// (k, 0) = c1 v1 + c2 v2 + (k1, k2) with c1 = round(k b2 / r), c2 = round(-k b1 / r), taken as
// (k G + 2^287) >> 288 with G = round(2^288 |b| / r): each c is within 1/2 + 2^-32 of the exact
// quotient, so |k1| <= (|a1| + |a2|)(1/2 + 2^-32) and |k2| <= (|b1| + |b2|)(1/2 + 2^-32), both < 2^126
// (the measured maximum over 3 x 10^5 scalars has 126 bits).  The loop takes 128 bits, and the host
// test asserts < 2^127 on every scalar it tries.
// Two's-complement words mod 2^160: A = first coordinates, B = second coordinates.
constexpr int G1_SPLIT_SHIFT_WORDS = 9;  // 288 bits
FQ_DEVCONST uint32_t G1_LAT_A1[5] = {0x7d4f1128u, 0x8211bbebu, 0xeeb859fcu, 0x6f4d8248u, 0x00000000u};
FQ_DEVCONST uint32_t G1_LAT_A2[5] = {0x94d213e3u, 0x89d32568u, 0x00000000u, 0x00000000u, 0x00000000u};
FQ_DEVCONST uint32_t G1_LAT_B1[5] = {0x6b2dec1du, 0x762cda97u, 0xffffffffu, 0xffffffffu, 0xffffffffu};
FQ_DEVCONST uint32_t G1_LAT_B2[5] = {0x1221250bu, 0x0be4e154u, 0xeeb859fdu, 0x6f4d8248u, 0x00000000u};
FQ_DEVCONST uint32_t G1_LAT_G1[6] = {0x149d5410u, 0x00ff6565u, 0x5398fd03u, 0xa773d2d2u, 0x4ccef014u, 0x00000002u};
FQ_DEVCONST uint32_t G1_LAT_G2[6] = {0x6eb9c714u, 0xc7e0b3d7u, 0xd91d232eu, 0x00000002u, 0x00000000u, 0x00000000u};

struct g1_glv {
    uint32_t k1[5], k2[5];  // |k1|, |k2| (word 4 is zero: asserted by the host test)
    bool neg1, neg2;
};

// c = (k g + 2^287) >> 288 as five words (k < 2^256, g < 2^162: c < 2^130)
FQ_FN void g1_round_quot(uint32_t c[5], const uint32_t k[8], const uint32_t g[6]) {
    uint32_t t[14];
#pragma unroll
    for (int i = 0; i < 14; i++) t[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint64_t cy = 0;
#pragma unroll
        for (int j = 0; j < 6; j++) {
            cy += (uint64_t)k[i] * g[j] + t[i + j];  // < 2^64
            t[i + j] = (uint32_t)cy;
            cy >>= 32;
        }
        t[i + 6] = (uint32_t)cy;
    }
    uint64_t cy = (uint64_t)(t[G1_SPLIT_SHIFT_WORDS - 1] >> 31);  // the rounding bit
#pragma unroll
    for (int i = 0; i < 5; i++) {
        cy += t[G1_SPLIT_SHIFT_WORDS + i];
        c[i] = (uint32_t)cy;
        cy >>= 32;
    }
}
// acc -= c m (mod 2^160)
FQ_FN void g1_mulsub160(uint32_t acc[5], const uint32_t c[5], const uint32_t m[5]) {
    uint32_t t[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 5; i++) {
        uint64_t cy = 0;
#pragma unroll
        for (int j = 0; j + i < 5; j++) {
            cy += (uint64_t)c[i] * m[j] + t[i + j];
            t[i + j] = (uint32_t)cy;
            cy >>= 32;
        }
    }
    int64_t br = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) {
        br += (int64_t)acc[i] - (int64_t)t[i];
        acc[i] = (uint32_t)br;
        br >>= 32;  // arithmetic: the borrow
    }
}
// |x| of a two's-complement value mod 2^160; returns its sign
FQ_FN bool g1_abs160(uint32_t x[5]) {
    bool neg = (x[4] >> 31) != 0;
    uint64_t cy = neg ? 1 : 0;
#pragma unroll
    for (int i = 0; i < 5; i++) {
        cy += neg ? (uint32_t)~x[i] : x[i];
        x[i] = (uint32_t)cy;
        cy >>= 32;
    }
    return neg;
}
FQ_FN void g1_glv_split(g1_glv& o, const uint32_t k[8]) {
    uint32_t c1[5], c2[5];
    g1_round_quot(c1, k, G1_LAT_G1);
    g1_round_quot(c2, k, G1_LAT_G2);
#pragma unroll
    for (int i = 0; i < 5; i++) {
        o.k1[i] = k[i];
        o.k2[i] = 0;
    }
    g1_mulsub160(o.k1, c1, G1_LAT_A1);
    g1_mulsub160(o.k1, c2, G1_LAT_A2);
    g1_mulsub160(o.k2, c1, G1_LAT_B1);
    g1_mulsub160(o.k2, c2, G1_LAT_B2);
    o.neg1 = g1_abs160(o.k1);
    o.neg2 = g1_abs160(o.k2);
}
// The loop's digit source: bit 127 of each half as a joint digit (bit 0: k1, bit 1: k2), then both
// shift left by one — static word indices only, so the halves stay in registers.
FQ_FN uint32_t g1_glv_next_digit(uint32_t k1[4], uint32_t k2[4]) {
    uint32_t d = (k1[3] >> 31) | ((k2[3] >> 31) << 1);
#pragma unroll
    for (int i = 3; i > 0; i--) {
        k1[i] = (k1[i] << 1) | (k1[i - 1] >> 31);
        k2[i] = (k2[i] << 1) | (k2[i - 1] >> 31);
    }
    k1[0] <<= 1;
    k2[0] <<= 1;
    return d;
}
FQ_FN uint32_t g1_next_bit256(uint32_t k[8]) {
    uint32_t d = k[7] >> 31;
#pragma unroll
    for (int i = 7; i > 0; i--) k[i] = (k[i] << 1) | (k[i - 1] >> 31);
    k[0] <<= 1;
    return d;
}

// ---------------------------------------------------------------------------- the group law
struct g1p { fq x, y, z; };  // Jacobian, z == 0: infinity (curve.go:10-12, 54-57)

// curve.go:143-172 (dbl-2009-l, a = 0; the curve's constant term does not occur); 7 products
FQ_FN g1p g1_dbl(const g1p& a) {
    fq A = fq_store(fq_mul(a.x, a.x));
    fq B = fq_store(fq_mul(a.y, a.y));
    fq C = fq_store(fq_mul(B, B));
    auto t = fq_add(a.x, B);
    fq d = fq_store(fq_mul_small<2>(fq_sub(fq_sub(fq_mul(t, t), A), C)));
    fq e = fq_store(fq_mul_small<3>(A));
    g1p r;
    r.x = fq_store(fq_sub(fq_mul(e, e), fq_mul_small<2>(d)));
    r.y = fq_store(fq_sub(fq_mul(e, fq_sub(d, r.x)), fq_mul_small<8>(C)));
    r.z = fq_store(fq_mul_small<2>(fq_mul(a.y, a.z)));
    return r;
}
// a + (bx, by, 1): curve.go:63-141 (add-2007-bl) with z2 = 1 (madd-2007-bl), 11 products, with the
// reference's branches: a at infinity -> b; equal points -> doubling; opposite points -> z = 0 by the
// formula itself (z3 = 2 z1 h).  (bx, by) is never infinity.
FQ_FN g1p g1_madd(const g1p& a, const fq& bx, const fq& by) {
    fq z1z1 = fq_store(fq_mul(a.z, a.z));
    fq u2 = fq_store(fq_mul(bx, z1z1));
    fq s2 = fq_store(fq_mul(by, fq_mul(a.z, z1z1)));
    fq h = fq_store(fq_sub(u2, a.x));
    fq t = fq_store(fq_sub(s2, a.y));
    bool ainf = fq_is_zero(a.z), same = fq_is_zero(h) && fq_is_zero(t);
    fq hh = fq_store(fq_mul(h, h));
    fq i = fq_store(fq_mul_small<4>(hh));
    fq j = fq_store(fq_mul(h, i));
    fq r = fq_store(fq_mul_small<2>(t));
    fq v = fq_store(fq_mul(a.x, i));
    g1p o;
    o.x = fq_store(fq_sub(fq_sub(fq_mul(r, r), j), fq_mul_small<2>(v)));
    o.y = fq_store(fq_sub(fq_mul(r, fq_sub(v, o.x)), fq_mul_small<2>(fq_mul(a.y, j))));
    auto zs = fq_add(a.z, h);
    o.z = fq_store(fq_sub(fq_sub(fq_mul(zs, zs), z1z1), hh));
    if (ainf) {
        o.x = bx;
        o.y = by;
        o.z = fq_one();
    } else if (same) {
        o = g1_dbl(a);
    }
    return o;
}

// G1.Unmarshal (bn256.go:120-158): coordinates < p, (0, 0) = infinity, else on the curve
// (curve.go:39-52).  Returns false for a malformed point.
FQ_FN bool g1_unmarshal(fq& x, fq& y, bool& inf, const uint8_t* s) {
    bool ok = fp_unmarshal(x, s);
    ok = fp_unmarshal(y, s + 32) && ok;
    inf = fq_is_zero(x) && fq_is_zero(y);
    if (ok && !inf) ok = fq_eq(fq_mul(y, y), fq_add(fq_mul(fq_mul(x, x), x), fq_const(FQ_THREE)));
    return ok;
}
FQ_FN void g1_zero64(uint8_t* out) {
#pragma unroll
    for (int i = 0; i < 64; i++) out[i] = 0;
}
// G1.Marshal (bn256.go:98-116) of the Jacobian point a: MakeAffine, montDecode, big-endian; 64 zero
// bytes for infinity.  The one inversion of an item.
FQ_FN void g1_marshal(uint8_t* out, const g1p& a) {
    bool inf = fq_is_zero(a.z);
    fq z = a.z;
    fq_cmov(z, fq_one(), inf);
    fq zi = fq_inv(z);
    fq zi2 = fq_store(fq_mul(zi, zi));
    fq ax = fq_store(fq_mul(a.x, zi2));
    fq ay = fq_store(fq_mul(a.y, fq_mul(zi2, zi)));
    if (inf) {
        g1_zero64(out);
    } else {
        fp_marshal(out, ax);
        fp_marshal(out + 32, ay);
    }
}

constexpr uint8_t G1_ST_OK = 0, G1_ST_BAD = 9;  // GSV_ST_OK, GSV_ST_BN_BAD_INPUT (include/gsv.h)

// bn256Add.Run (contracts.go:274-289) on one 128-byte record x1 || y1 || x2 || y2
FQ_FN uint8_t g1_add_item(uint8_t* out, const uint8_t* in) {
    fq x1, y1, x2, y2;
    bool inf1, inf2;
    bool ok = g1_unmarshal(x1, y1, inf1, in);
    ok = g1_unmarshal(x2, y2, inf2, in + 64) && ok;
    if (!ok) {
        g1_zero64(out);
        return G1_ST_BAD;
    }
    // an infinite second operand: add P1 to "infinity" instead, the same code path
    g1p a{x1, y1, fq_one()};
    fq bx = x2, by = y2;
    if (inf1) a.z = fq_zero();
    if (inf2) {
        a.z = fq_zero();
        bx = x1;
        by = y1;
    }
    g1p s = g1_madd(a, bx, by);
    if (inf1 && inf2) s.z = fq_zero();
    g1_marshal(out, s);
    return G1_ST_OK;
}

// bn256ScalarMul.Run (contracts.go:297-312) on one 96-byte record x || y || k
template <bool BITSERIAL>
FQ_FN uint8_t g1_mul_item(uint8_t* out, const uint8_t* in) {
    fq x, y;
    bool inf;
    if (!g1_unmarshal(x, y, inf, in)) {
        g1_zero64(out);
        return G1_ST_BAD;
    }
    uint32_t k[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint8_t* q = in + 64 + 28 - 4 * i;
        k[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
    }
    if (inf) {  // k * infinity
        g1_zero64(out);
        return G1_ST_OK;
    }
    g1p sum{fq_zero(), fq_one(), fq_zero()};
    if constexpr (BITSERIAL) {
#if defined(__HIPCC__)
#pragma unroll 1
#endif
        for (int b = 0; b < 256; b++) {
            g1p t = g1_dbl(sum);
            if (g1_next_bit256(k)) sum = g1_madd(t, x, y);
            else sum = t;
        }
    } else {
        g1_glv g;
        g1_glv_split(g, k);
        uint32_t k1[4], k2[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            k1[i] = g.k1[i];
            k2[i] = g.k2[i];
        }
        // T1 = (x, +-y), T2 = (beta x, +-y): distinct x (beta != 1, and no point of G1 has x = 0), so
        // T3 = T1 + T2 is the plain chord (mmadd-2007-bl, z1 = z2 = 1): z3 = 2 h != 0
        fq y1 = y, y2 = y;
        fq ny = fq_store(fq_neg(y));
        fq_cmov(y1, ny, g.neg1);
        fq_cmov(y2, ny, g.neg2);
        fq x2 = fq_store(fq_mul(x, fq_const(FQ_XI_PSQ1_3)));
        fq h = fq_store(fq_sub(x2, x));
        fq hh = fq_store(fq_mul(h, h));
        fq i4 = fq_store(fq_mul_small<4>(hh));
        fq j = fq_store(fq_mul(h, i4));
        fq r = fq_store(fq_mul_small<2>(fq_sub(y2, y1)));
        fq v = fq_store(fq_mul(x, i4));
        fq x3 = fq_store(fq_sub(fq_sub(fq_mul(r, r), j), fq_mul_small<2>(v)));
        fq y3 = fq_store(fq_sub(fq_mul(r, fq_sub(v, x3)), fq_mul_small<2>(fq_mul(y1, j))));
        fq z3 = fq_store(fq_mul_small<2>(h));
        // T1, T2 at the common Z = z3
        fq zz = fq_store(fq_mul(z3, z3));
        fq zzz = fq_store(fq_mul(zz, z3));
        fq tx1 = fq_store(fq_mul(x, zz));
        fq tx2 = fq_store(fq_mul(x2, zz));
        fq ty1 = fq_store(fq_mul(y1, zzz));
        fq ty2 = ty1;
        fq_cmov(ty2, fq_store(fq_neg(ty1)), g.neg1 != g.neg2);
#if defined(__HIPCC__)
#pragma unroll 1
#endif
        for (int b = 0; b < 128; b++) {
            g1p t = g1_dbl(sum);
            uint32_t d = g1_glv_next_digit(k1, k2);
            if (d) {
                fq bx = tx1, by = ty1;
                fq_cmov(bx, tx2, d == 2);
                fq_cmov(by, ty2, d == 2);
                fq_cmov(bx, x3, d == 3);
                fq_cmov(by, y3, d == 3);
                sum = g1_madd(t, bx, by);
            } else {
                sum = t;
            }
        }
        sum.z = fq_store(fq_mul(sum.z, z3));  // back from y^2 = x^3 + 3 z3^6
    }
    g1_marshal(out, sum);
    return G1_ST_OK;
}

}  // namespace bn
}  // namespace gsv
