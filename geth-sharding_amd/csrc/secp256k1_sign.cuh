// ECDSA signing on the comb: the signature itself (crypto.Sign's, ecsign.hip) and the synthetic
// signer that makes bench / test data on the device (ecrecover.hip k_synth_sign, notary.hip
// k_notary_synth).
#pragma once
#include "keccak_dev.cuh"
#include "secp256k1_comb.cuh"
#include "secp256k1_point.cuh"

namespace gsv {

// ---------------------------------------------------------------------------- synthetic signer
// Bench/test data generator (signing is not on the validation path): key_i, msg_i, nonce_i are
// Keccak-256 of (le64(seed) || le64(i) || tag), keys/nonces reduced mod n (0 -> 1).
GSV_DI void derive32(uint32_t out_be_limbs[8], uint64_t seed, uint64_t i, uint32_t tag3) {
    uint64_t a[25];
#pragma unroll
    for (int k = 0; k < 25; k++) a[k] = 0;
    a[0] = seed;
    a[1] = i;
    a[2] = (uint64_t)(tag3 & 0xFFFFFFu) | (0x01ull << 24);
    a[16] = 0x8000000000000000ULL;
    keccakf(a);
    // hash bytes as a big-endian 256-bit number -> limbs
#pragma unroll
    for (int j = 0; j < 4; j++) {
        out_be_limbs[7 - 2 * j] = __builtin_bswap32((uint32_t)a[j]);
        out_be_limbs[6 - 2 * j] = __builtin_bswap32((uint32_t)(a[j] >> 32));
    }
}

// The signature itself (libsecp256k1/src/ecdsa_impl.h secp256k1_ecdsa_sig_sign): R = k G, r = R.x mod n,
// s = (m + r d) / k, low-s normalised, recid = (R.x >= n ? 2 : 0) | (R.y odd), bit 0 flipped with s.
// d, k in [1, n), m = the message as limbs (any 256-bit value; reduced here, where s needs it).  One comb
// multiplication.  r or s may come out zero: the caller's to test (crypto.Sign's retry; the synthetic
// signer does not).
GSV_DI void ecdsa_sign_core(uint32_t r_out[8], uint32_t s_out[8], uint32_t& recid, const sc& d, const sc& k,
                            const uint32_t m[8], const uint4* __restrict__ gtab) {
    gej9 R;
    bool rinf;
    comb_mul_g9(R, rinf, k, gtab);
    fe rx, ry;
    gej9_to_affine_words(rx, ry, R);
    recid = ry.v[0] & 1u;
    sc r;
    bool over = !limbs_lt(rx.v, SN);
    sc_cond_sub_n(r.v, rx.v, 0);
    if (over) recid |= 2u;
    // s = k^-1 (m + r d)
    sc kinv, s, t, mr;
    modinv30_words_ct(kinv.v, k.v, MI30_N);  // the nonce is secret: constant-time divsteps
    sc_cond_sub_n(mr.v, m, 0);               // msg mod n (msg < 2^256 < 2n)
    sc_mul(t, r, d);
    sc_add(t, t, mr);
    sc_mul(s, kinv, t);
    if (sc_is_high(s)) {
        sc_neg(s, s);
        recid ^= 1u;
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        r_out[i] = r.v[i];
        s_out[i] = s.v[i];
    }
}

// The synthetic signer's signature with an explicit nonce: d, k are reduced mod n here (0 -> 1, this
// signer's rule alone).  (px, py) = d*G.  m = message as limbs (any 256-bit value).
GSV_DI void ecdsa_sign(uint32_t r_out[8], uint32_t s_out[8], uint32_t& recid, fe& px, fe& py, sc d, sc k,
                       const uint32_t m[8], const uint4* __restrict__ gtab) {
    sc_cond_sub_n(d.v, d.v, 0);
    sc_cond_sub_n(k.v, k.v, 0);
    if (sc_is_zero(d)) d.v[0] = 1;
    if (sc_is_zero(k)) k.v[0] = 1;
    gej9 P;
    bool pinf;
    comb_mul_g9(P, pinf, d, gtab);
    gej9_to_affine_words(px, py, P);
    ecdsa_sign_core(r_out, s_out, recid, d, k, m, gtab);
}

}  // namespace gsv
