// secp256k1 point helpers shared by the kernels: constants as fe9, the curve test, the harmless
// stand-in for an invalid point, the Jacobian -> affine conversions and the public-key / address
// store.  Field elements are fe9 (secp256k1_fe9.cuh); the magnitude of every intermediate is noted.
//
// A unit that also runs a GLV ladder includes secp256k1_glv.cuh BEFORE this header (it says why).
#pragma once
#include "keccak_dev.cuh"
#include "secp256k1_scalar.cuh"
#include "secp256k1_fe9.cuh"
#include "modinv30.cuh"

// waves per SIMD the curve kernels (recovery, verification, ECDH, signing) are compiled for
// (register budget 512 / waves)
#define GSV_ECR_WAVES 2

namespace gsv {

GSV_DI void fe9_from_const(fe9& r, const uint32_t c[8]) {
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = c[i];
    fe9_from_words(r, w);
}

// ---------------------------------------------------------------------------- the curve test
// c = x^3 + 7 (x magnitude 1): limb 0 < 2^29 + 7, the others as a product's output
GSV_DI void curve_rhs9(fe9& c, const fe9& x) {
    fe9 t;
    fe9_sqr(t, x);
    fe9_mul(c, t, x);
    c.v[0] += 7u;
}
// y^2 == x^3 + 7 (x, y magnitude 1): a canonical compare
GSV_DI bool on_curve9(const fe9& x, const fe9& y) {
    fe9 c, yy;
    curve_rhs9(c, x);
    fe9_normalize_full(c);
    fe9_sqr(yy, y);
    fe9_normalize_full(yy);
    return fe9_eq_canon(yy, c);
}

// An invalid item runs the whole schedule on the generator (and sc_set_one_unless's scalar 1): no
// lane leaves a ladder early.
GSV_DI void ge9_set_g_unless(fe9& x, fe9& y, bool ok) {
    fe9 gx, gy;
    fe9_from_const(gx, GX);
    fe9_from_const(gy, GY);
    fe9_cmov(x, gx, !ok);
    fe9_cmov(y, gy, !ok);
}

// ---------------------------------------------------------------------------- Jacobian -> affine
// Jacobian -> affine canonical 8 x 32-bit words (variable time)
GSV_DI void gej9_to_affine_words(fe& ax, fe& ay, const gej9& q) {
    fe9 zi, zi2, x, y;
    {
        fe9 z = q.z;
        fe9_normalize_full(z);
        uint32_t zw[8], iw[8];
        fe9_to_words(zw, z);
        modinv30_words(iw, zw, MI30_P);  // Z^-1 mod p (safegcd)
        fe9_from_words(zi, iw);
    }
    fe9_sqr(zi2, zi);
    fe9_mul(x, q.x, zi2);
    fe9_mul(zi2, zi2, zi);
    fe9_mul(y, q.y, zi2);
    fe9_normalize_full(x);
    fe9_normalize_full(y);
    fe9_to_words(ax.v, x);
    fe9_to_words(ay.v, y);
}
// The same for a Z that depends on a secret scalar, in two steps (ECDH's shared X needs no Y):
// Z^-1 by the CONSTANT-TIME divsteps (the variable-time inversion's trip count would show in the
// wave's time), x = X Z^-2 in canonical words with zi2 = Z^-2 kept for gej9_affine_y_ct.
GSV_DI void gej9_affine_x_ct(fe& ax, fe9& zi, fe9& zi2, const gej9& q) {
    {
        fe9 z = q.z;
        fe9_normalize_full(z);
        uint32_t zw[8], iw[8];
        fe9_to_words(zw, z);
        modinv30_words_ct(iw, zw, MI30_P);
        fe9_from_words(zi, iw);
    }
    fe9 x;
    fe9_sqr(zi2, zi);
    fe9_mul(x, q.x, zi2);
    fe9_normalize_full(x);
    fe9_to_words(ax.v, x);
}
// y = Y Z^-3 in canonical words
GSV_DI void gej9_affine_y_ct(fe& ay, const gej9& q, const fe9& zi, const fe9& zi2) {
    fe9 zi3, y;
    fe9_mul(zi3, zi2, zi);
    fe9_mul(y, q.y, zi3);
    fe9_normalize_full(y);
    fe9_to_words(ay.v, y);
}

// ---------------------------------------------------------------------------- public key, address
// pub65 (may be null): 04 || X || Y; addr20 (may be null): Keccak256(X || Y)[12:]; zeros unless ok
GSV_DI void store_pub_addr(uint8_t* pub65, uint8_t* addr20, bool ok, const fe& qx, const fe& qy) {
    if (pub65) {
        pub65[0] = ok ? 4 : 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            uint32_t xv = ok ? qx.v[7 - i] : 0u, yv = ok ? qy.v[7 - i] : 0u;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                pub65[1 + 4 * i + b] = (uint8_t)(xv >> (24 - 8 * b));
                pub65[33 + 4 * i + b] = (uint8_t)(yv >> (24 - 8 * b));
            }
        }
    }
    if (addr20) {
        uint32_t h[8];
        keccak256_xy(h, qx.v, qy.v);  // one permutation, in digest form
        // hash bytes 12..31 = words 3..7 (little-endian byte order within words)
#pragma unroll
        for (int w = 3; w < 8; w++)
#pragma unroll
            for (int b = 0; b < 4; b++) addr20[(w - 3) * 4 + b] = ok ? (uint8_t)(h[w] >> (8 * b)) : 0;
    }
}

}  // namespace gsv
