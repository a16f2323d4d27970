// Batched secp256k1 ECDSA verification with a known key, and public-key parsing, on gfx950 — one item
// per lane.
//
// Semantics restated from the reference's cgo path (bit-exact verdicts):
//   crypto/secp256k1/ext.h secp256k1_ext_ecdsa_verify     parse_compact -> pubkey_parse -> ecdsa_verify
//   crypto/secp256k1/ext.h secp256k1_ext_reencode_pubkey  pubkey_parse -> pubkey_serialize
//   libsecp256k1/src/secp256k1.c ecdsa_signature_parse_compact: r, s >= n -> invalid (not reduced);
//                         ecdsa_verify: s > n/2 -> invalid (the malleability rule), m = msg32 mod n
//   libsecp256k1/src/eckey_impl.h eckey_pubkey_parse: 33 bytes 02/03 | 65 bytes 04/06/07, x, y < p,
//                         on the curve, 06/07 with y of the prefix's parity
//   libsecp256k1/src/ecdsa_impl.h ecdsa_sig_verify: r, s != 0; X = (m/s) G + (r/s) P; X != O;
//                         r Z^2 == X_x or (r < p - n and (r + n) Z^2 == X_x), both projective
//
// Algorithm: the recovery kernels' parts (secp256k1_glv.cuh, secp256k1_comb.cuh) on a caller-chosen point.  u2 P is the GLV
// w = 4 ladder (glv_mul_point) on the parsed key, u1 G the 20-bit comb; one general Jacobian add that
// produces X3 and Z3 only, then the projective comparison.  No square root for an uncompressed key,
// no inversion mod p anywhere in k_ecverify: recovery's exponentiation by (p - 3) / 4 has no
// counterpart.  A compressed key costs one square root (fe9_sqrt), taken behind a wave-uniform guard.
// An invalid item runs the whole schedule on harmless inputs (the generator, r = s = 1) and has its
// verdict forced to 0 at the end: no lane leaves the ladder early.
#include "opcount.cuh"
#include "secp256k1_glv.cuh"  // before the other secp256k1 headers
#include "secp256k1_comb.cuh"
#include "secp256k1_point.cuh"

namespace gsv {

// ---------------------------------------------------------------------------- key parse
// row: 65 bytes (a 33-byte key is followed by padding that is not read as key material), len: the
// key's length.  Returns whether the key parses (eckey_pubkey_parse); then (x, y) is the point, both
// canonical (limbs of a value < p).  When it does not parse (x, y) is the generator.
GSV_DI bool pubkey_parse9(fe9& x, fe9& y, const uint8_t* __restrict__ row, uint32_t len) {
    const uint32_t prefix = row[0];
    uint32_t xw[8], yw[8];
    load32_be(xw, row + 1);
    load32_be(yw, row + 33);
    const bool comp = len == 33u && (prefix == 2u || prefix == 3u);
    const bool full = len == 65u && (prefix == 4u || prefix == 6u || prefix == 7u);
    bool ok = (comp || full) && limbs_lt(xw, FP);
    fe9_from_words(x, xw);
    fe9_from_words(y, yw);
    fe9 c;
    curve_rhs9(c, x);                        // x^3 + 7, shared by the root and the curve test
    if (FE9_ANY(comp)) {                     // wave-uniform: no lane pays the root for a 65-byte key
        fe9 root;
        bool sq = fe9_sqrt(root, c);
        fe9_normalize_full(root);
        fe9 nr;
        fe9_neg<1>(nr, root);
        fe9_normalize_full(nr);              // root != 0: 7 is not a cube's negative on this curve
        fe9_cmov(root, nr, (root.v[0] & 1u) != (prefix & 1u));
        fe9_cmov(y, root, comp);
        ok = ok && (!comp || sq);
    }
    // the 65-byte forms: y < p, y^2 = x^3 + 7, and the hybrid prefixes' parity
    {
        fe9 yy;
        fe9_sqr(yy, y);
        fe9_normalize_full(yy);
        fe9 cc = c;
        fe9_normalize_full(cc);
        bool on = fe9_eq_canon(yy, cc);
        bool par = prefix == 4u || (yw[0] & 1u) == (prefix & 1u);
        ok = ok && (!full || (limbs_lt(yw, FP) && on && par));
    }
    ge9_set_g_unless(x, y, ok);
    return ok;
}

// ---------------------------------------------------------------------------- the final add
// X3 and Z3 of p1 + p2 (Jacobian; X, Y magnitude 1; Z1 magnitude <= 2, Z2 magnitude 1), add-1998-cmo
// without its Y3: U1 = X1 Z2^2, U2 = X2 Z1^2, S1 = Y1 Z2^3, S2 = Y2 Z1^3, H = U2 - U1, rr = S2 - S1,
// X3 = rr^2 - H^3 - 2 U1 H^2, Z3 = Z1 Z2 H.  Returns false when the sum is the identity.  The
// exceptional cases sit behind wave-uniform guards:
//   p1 = O -> p2;  p2 = O -> p1;  both -> O;  H == 0 and rr == 0 -> 2 p2;  H == 0, rr != 0 -> O.
GSV_DI bool gej9_add_xz(fe9& x3, fe9& z3, const gej9& p1, bool p1inf, const gej9& p2, bool p2inf) {
    fe9 z1z1, z2z2, u1, h, s1, s2, rr, t;
    fe9_sqr(z1z1, p1.z);                     // 2 -> 1
    fe9_sqr(z2z2, p2.z);                     // 1
    fe9_mul(u1, p1.x, z2z2);                 // 1
    fe9_neg<1>(t, u1);                       // limbs < 2^30
    fe9_mul_add(h, p2.x, z1z1, t);           // H = U2 - U1, 1 (a product's output)
    fe9_mul(s1, p1.y, p2.z);
    fe9_mul(s1, s1, z2z2);                   // S1, 1
    fe9_mul(s2, p2.y, p1.z);                 // 1*2
    fe9_neg<1>(t, s1);
    fe9_mul_add(rr, s2, z1z1, t);            // rr = S2 - S1, 1
    fe9 hh, hhh, v;
    fe9_sqr(hh, h);
    fe9_mul(hhh, h, hh);                     // H^3
    fe9_mul(v, u1, hh);                      // V = U1 H^2
    fe9_negsum3<3>(t, hhh, v, v);            // -(H^3 + 2V), limbs < 2^31
    fe9_sqr_add(x3, rr, t);                  // X3, 1
    fe9_mul(t, p1.z, p2.z);                  // 2*1
    fe9_mul(z3, t, h);                       // Z3 = Z1 Z2 H, 1
    bool inf = p1inf && p2inf;
    const bool exc = !p1inf && !p2inf && fe9_is_zero_weak(h);
    if (FE9_ANY(exc)) {  // p1 == +-p2 (rare)
        bool same = fe9_is_zero(rr);
        gej9 d;
        gej9_dbl(d, p2);
        fe9_cmov(x3, d.x, exc);
        fe9_cmov(z3, d.z, exc);
        inf = inf || (exc && !same);
    }
    if (FE9_ANY(p1inf)) {  // u1 G = O (u1 == 0): the sum is u2 P
        fe9_cmov(x3, p2.x, p1inf);
        fe9_cmov(z3, p2.z, p1inf);
    }
    if (FE9_ANY(p2inf)) {  // the ladder's identity flag: the sum is u1 G
        fe9 z1 = p1.z;
        fe9_normalize_weak(z1);
        fe9_cmov(x3, p1.x, p2inf);
        fe9_cmov(z3, z1, p2inf);
    }
    return !inf;
}

// ---------------------------------------------------------------------------- verification core
// msg / r / s: 256-bit values as little-endian limbs; (px, py), keyok: pubkey_parse9's outputs.
GSV_DI bool verify_core(const uint32_t msg[8], const uint32_t r[8], const uint32_t s[8], const fe9& px,
                        const fe9& py, bool keyok, const uint4* __restrict__ gtab,
                        uint32_t* __restrict__ ltab) {
    sc rs, ss, m;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        rs.v[i] = r[i];
        ss.v[i] = s[i];
    }
    // parse_compact: overflow is invalid, not reduced; sig_verify: zero is invalid; s <= n/2
    const bool sigok = limbs_lt(r, SN) && limbs_lt(s, SN) && !sc_is_zero(rs) && !sc_is_zero(ss) &&
                       !sc_is_high(ss);
    // an invalid signature runs as r = s = 1
    sc_set_one_unless(rs, sigok);
    sc_set_one_unless(ss, sigok);
    sc_cond_sub_n(m.v, msg, 0);  // msg mod n (msg < 2^256 < 2n); may be 0

    // u1 = m / s, u2 = r / s
    sc sn, u1, u2;
    modinv30_words(sn.v, ss.v, MI30_N);  // s^-1 mod n (safegcd)
    sc_mul(u1, sn, m);
    sc_mul(u2, sn, rs);

    gej9 acc;  // u2 P: u2 != 0 and P has order n, so the flag stays clear; honoured all the same
    bool ainf;
    glv_mul_point(acc, ainf, u2, px, py, ltab);

    gej9 accg;  // u1 G; u1 == 0 gives ginf
    bool ginf;
    comb_mul_g9(accg, ginf, u1, gtab);

    fe9 x3, z3;
    bool ok = gej9_add_xz(x3, z3, accg, ginf, acc, ainf) && sigok && keyok;

    // r Z^2 == X, or r < p - n and (r + n) Z^2 == X
    fe9 zz, rf, t;
    fe9_sqr(zz, z3);
    fe9_from_words(rf, rs.v);
    fe9_mul(t, rf, zz);
    fe9_normalize_full(t);
    fe9_normalize_full(x3);
    bool eq = fe9_eq_canon(t, x3);
    const bool wrap = limbs_lt(rs.v, P_MINUS_N);
    if (FE9_ANY(wrap)) {  // r < p - n = 2^128.3: one r in 2^127.7
        uint32_t w[8];
        uint64_t c = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            c = (uint64_t)rs.v[i] + SN[i] + hi32(c);
            w[i] = lo32(c);
        }
        fe9_from_words(rf, w);  // r + n < p for the lanes that use it
        fe9_mul(t, rf, zz);
        fe9_normalize_full(t);
        eq = eq || (wrap && fe9_eq_canon(t, x3));
    }
    return ok && eq;
}

// ---------------------------------------------------------------------------- kernels
// pub65: n rows of 65 bytes, publen: the key lengths (33 or 65; anything else is an invalid key)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(GSV_ECR_WAVES, GSV_ECR_WAVES))) void k_ecverify(
    const uint8_t* __restrict__ msg32, const uint8_t* __restrict__ sig64, const uint8_t* __restrict__ pub65,
    const uint8_t* __restrict__ publen, uint32_t n, const uint4* __restrict__ gtab, uint8_t* __restrict__ ok) {
    GSV_LTAB_DECL;
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* sg = sig64 + (size_t)i * 64;
    uint32_t msg[8], r[8], s[8];
    load32_be(msg, msg32 + (size_t)i * 32);
    load32_be(r, sg);
    load32_be(s, sg + 32);
    fe9 px, py;
    bool keyok = pubkey_parse9(px, py, pub65 + (size_t)i * 65, publen[i]);
    bool good = verify_core(msg, r, s, px, py, keyok, gtab, GSV_LTAB_LANE);
    ok[i] = good ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_pubkey_parse(const uint8_t* __restrict__ pub65,
                                                      const uint8_t* __restrict__ publen, uint32_t n,
                                                      uint8_t* __restrict__ out65, uint8_t* __restrict__ ok) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe9 px, py;
    bool good = pubkey_parse9(px, py, pub65 + (size_t)i * 65, publen[i]);
    fe qx, qy;
    fe9_to_words(qx.v, px);
    fe9_to_words(qy.v, py);
    store_pub_addr(out65 + (size_t)i * 65, nullptr, good, qx, qy);
    ok[i] = good ? 1 : 0;
}

// ---------------------------------------------------------------------------- launchers
hipError_t launch_ecverify(const uint8_t* msg32, const uint8_t* sig64, const uint8_t* pub65, const uint8_t* publen,
                           uint32_t n, const uint4* gtab, uint8_t* ok, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ecverify, dim3((n + 255) / 256), dim3(256), 0, st, msg32, sig64, pub65, publen, n, gtab,
                       ok);
    return hipGetLastError();
}

hipError_t launch_pubkey_parse(const uint8_t* pub65, const uint8_t* publen, uint32_t n, uint8_t* out65, uint8_t* ok,
                               hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pubkey_parse, dim3((n + 255) / 256), dim3(256), 0, st, pub65, publen, n, out65, ok);
    return hipGetLastError();
}

}  // namespace gsv

GSV_OPCOUNT_READER(ecverify)
