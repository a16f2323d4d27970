// Batched secp256k1 ScalarMult and ECDH shared secrets on gfx950 — one item per lane.
//
// Semantics restated from the reference's cgo path (bit-exact results, one deliberate divergence):
//   crypto/secp256k1/ext.h secp256k1_ext_scalar_mul      fe_set_b32 x 2 (return value ignored: a
//                         coordinate >= p is reduced mod p), ge_set_xy (no curve check),
//                         scalar_set_b32: a scalar of 0 or >= n returns 0 and leaves the point alone;
//                         else ecmult_const, ge_set_gej, normalize, X || Y
//   crypto/secp256k1/curve.go:221-259 ScalarMult / ScalarBaseMult: 0 becomes (nil, nil)
//   crypto/ecies/ecies.go:121-138 GenerateShared: the shared secret is X
//   crypto/ecies/ecies.go:264-277 the keys of ECIES_AES128_SHA256 with s1 empty (ecies_kdf.cuh)
// The divergence: a point that is not on the curve is refused (GSV_ST_INVALID_CURVE), where the reference
// returns the output of its addition formulas on another curve (include/gsv.h says why).
//
// Algorithm: the curve check (canonical compare, secp256k1_point.cuh on_curve9), secp256k1_glv.cuh's GLV w = 4
// ladder (glv_mul_point: a uniform schedule of odd signed digits, no skipped adds) on the caller's
// point, one CONSTANT-TIME safegcd inversion mod p for the affine result (Z depends on the secret
// scalar: the variable-time inversion's trip count would show in the wave's time), a full normalise
// and a big-endian store.  The shared X alone skips the Y product; the ECIES keys add two SHA-256
// compressions.  No comb multiplication, no inversion mod n.  An invalid item runs the whole schedule on
// harmless inputs (the generator, k = 1) and has its outputs zeroed at the end: no lane leaves the
// ladder early.
#include "opcount.cuh"
#include "gsv_internal.h"
#include "secp256k1_glv.cuh"  // before the other secp256k1 headers
#include "secp256k1_point.cuh"
#include "ecies_kdf.cuh"

namespace gsv {

// point64: n rows X || Y, scalar32: n big-endian scalars.  Outputs, each may be null (wave-uniform):
// xy64 = X || Y of k P, x32 = X alone, keys48 = Ke || Km derived from X.  A failed item's rows are zero.
// Two waves per SIMD, as k_ecverify: the ladder's live state and the LDS table are the same.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(GSV_ECR_WAVES, GSV_ECR_WAVES))) void k_ecdh(
    const uint8_t* __restrict__ point64, const uint8_t* __restrict__ scalar32, uint32_t n,
    uint8_t* __restrict__ xy64, uint8_t* __restrict__ x32, uint8_t* __restrict__ keys48,
    uint8_t* __restrict__ status) {
    GSV_LTAB_DECL;
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    sc k;
    fe9 px, py;
    {
        uint32_t xw[8], yw[8];
        load32_be(xw, point64 + (size_t)i * 64);
        load32_be(yw, point64 + (size_t)i * 64 + 32);
        load32_be(k.v, scalar32 + (size_t)i * 32);
        // fe_set_b32 with its verdict ignored: a coordinate >= p (< 2^256 < 2p) is reduced
        fe9_from_words(px, xw);
        fe9_from_words(py, yw);
        fe9_normalize_full(px);
        fe9_normalize_full(py);
    }
    // scalar_set_b32's overflow and scalar_is_zero: the reference's only failure
    const bool scalar_ok = seckey_ok(k);
    const bool curve_ok = on_curve9(px, py);
    const bool ok = scalar_ok && curve_ok;
    // an invalid item runs as 1 * G
    ge9_set_g_unless(px, py, ok);
    // (sc_set_one_unless, written out: the call changes this kernel's instruction schedule)
#pragma unroll
    for (int j = 0; j < 8; j++) k.v[j] = ok ? k.v[j] : (j == 0 ? 1u : 0u);

    gej9 acc;  // k P: k in [1, n) and P of order n, so the flag stays clear; honoured all the same
    bool ainf;
    glv_mul_point(acc, ainf, k, px, py, GSV_LTAB_LANE);
    const bool good = ok && !ainf;

    // affine by the constant-time inversion: Z depends on the secret scalar
    fe9 zi, zi2;
    fe xa;
    gej9_affine_x_ct(xa, zi, zi2, acc);
    uint32_t xo[8];
#pragma unroll
    for (int j = 0; j < 8; j++) xo[j] = good ? xa.v[j] : 0u;

    if (xy64) {  // wave-uniform: ScalarMult's Y
        fe ya;
        gej9_affine_y_ct(ya, acc, zi, zi2);
        uint32_t yo[8];
#pragma unroll
        for (int j = 0; j < 8; j++) yo[j] = good ? ya.v[j] : 0u;
        limbs_to_be(xy64 + (size_t)i * 64, xo);
        limbs_to_be(xy64 + (size_t)i * 64 + 32, yo);
    }
    if (x32) limbs_to_be(x32 + (size_t)i * 32, xo);
    if (keys48) {  // wave-uniform
        // limbs are the big-endian words in reverse order (ecies_kdf.cuh)
        uint32_t xw[8], ke[4], km[8];
#pragma unroll
        for (int j = 0; j < 8; j++) xw[j] = xo[7 - j];
        ecies_kdf_keys(ke, km, xw);
        uint8_t* o = keys48 + (size_t)i * 48;
#pragma unroll
        for (int j = 0; j < 12; j++) {
            uint32_t v = j < 4 ? ke[j] : km[j - 4];
            v = good ? v : 0u;
#pragma unroll
            for (int b = 0; b < 4; b++) o[4 * j + b] = (uint8_t)(v >> (24 - 8 * b));
        }
    }
    // the scalar rule first: it is the reference's only failure
    status[i] = (uint8_t)(!scalar_ok || (curve_ok && ainf) ? GSV_ST_INVALID_KEY
                                                           : !curve_ok ? GSV_ST_INVALID_CURVE : GSV_ST_OK);
}

// ---------------------------------------------------------------------------- launcher
hipError_t launch_ecdh(const uint8_t* point64, const uint8_t* scalar32, uint32_t n, uint8_t* xy64, uint8_t* x32,
                       uint8_t* keys48, uint8_t* status, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ecdh, dim3((n + 255) / 256), dim3(256), 0, st, point64, scalar32, n, xy64, x32, keys48,
                       status);
    return hipGetLastError();
}

}  // namespace gsv

GSV_OPCOUNT_READER(ecdh)
