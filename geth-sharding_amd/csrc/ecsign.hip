// Batched crypto.Sign and public-key derivation on gfx950 — one item per lane.
//
// Semantics restated from the reference's cgo path (bit-exact signatures):
//   crypto/secp256k1/secp256.go:70-99 Sign: secp256k1_ec_seckey_verify (a key of 0 or >= n is
//                         ErrInvalidKey), secp256k1_ecdsa_sign_recoverable with
//                         secp256k1_nonce_function_rfc6979 and no extra data, serialize_compact: [R || S || recid]
//   libsecp256k1/src/modules/recovery/main_impl.h ecdsa_sign_recoverable: counter c = 0, 1, ...:
//                         k = nonce(msg32, key, c); k = 0 or k >= n -> next c; sig_sign; r = 0 or
//                         s = 0 -> next c.  The message enters the nonce as its raw 32 bytes and the
//                         signature reduced mod n.
//   libsecp256k1/src/ecdsa_impl.h ecdsa_sig_sign: R = k G, r = R.x mod n, s = (m + r d) / k, low s,
//                         recid = (R.x >= n ? 2 : 0) | (R.y odd), bit 0 flipped when s is negated
//   libsecp256k1/src/secp256k1.c ec_pubkey_create: the same key rule, then d G
//
// Algorithm: the nonce of rfc6979_dev.cuh (16 SHA-256 compressions at counter 0; a retry starts the
// generator again, as the reference does, so that none of its state occupies registers through the curve
// arithmetic), then secp256k1_sign.cuh's ecdsa_sign_core: one 20-bit comb
// multiplication over the context's G table, one inversion mod p for the affine R, the constant-time
// safegcd inversion of the nonce mod n.  No GLV ladder, so no LDS table.  An item with an invalid key
// runs the whole schedule on the key 1 and has its output zeroed at the end: no lane leaves early.
#include "opcount.cuh"
#include "secp256k1_comb.cuh"
#include "secp256k1_sign.cuh"
#include "rfc6979_dev.cuh"

namespace gsv {

// compiled for two waves per SIMD (256 registers), as k_synth_sign comes out on its own
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(GSV_ECR_WAVES, GSV_ECR_WAVES))) void k_ecsign(
    const uint8_t* __restrict__ msg32, const uint8_t* __restrict__ seckey32, uint32_t n,
    const uint4* __restrict__ gtab, uint8_t* __restrict__ sig65, uint8_t* __restrict__ status) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    sc d;
    uint32_t m[8];
    load32_be(d.v, seckey32 + (size_t)i * 32);
    load32_be(m, msg32 + (size_t)i * 32);
    const bool keyok = seckey_ok(d);
    sc_set_one_unless(d, keyok);
    uint32_t r[8], s[8], recid, counter = 0;
    bool done;
#pragma unroll 1
    do {
        sc k;
        {
            // limbs are the big-endian words in reverse order (rfc6979_dev.cuh)
            uint32_t kw[8], mw[8], nw[8];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                kw[j] = d.v[7 - j];
                mw[j] = m[7 - j];
            }
            rfc6979_nonce(nw, kw, mw, counter);
#pragma unroll
            for (int j = 0; j < 8; j++) k.v[7 - j] = nw[j];
        }
        // a nonce of 0 or >= n is passed over (2^-128): the lane signs with 1 and discards the result
        const bool kok = seckey_ok(k);
        sc_set_one_unless(k, kok);
        ecdsa_sign_core(r, s, recid, d, k, m, gtab);
        done = kok && !limbs_zero(r) && !limbs_zero(s);
        counter++;
    } while (!done);
    uint8_t* sg = sig65 + (size_t)i * 65;
    if (!keyok) {
#pragma unroll
        for (int j = 0; j < 8; j++) r[j] = s[j] = 0;
        recid = 0;
    }
    limbs_to_be(sg, r);
    limbs_to_be(sg + 32, s);
    sg[64] = (uint8_t)recid;
    status[i] = keyok ? GSV_ST_OK : GSV_ST_INVALID_KEY;
}

// pub65: 04 || X || Y of d G; addr20 (may be null): Keccak256(X || Y)[12:]
__global__ __launch_bounds__(256) void k_pubkey_create(const uint8_t* __restrict__ seckey32, uint32_t n,
                                                       const uint4* __restrict__ gtab, uint8_t* __restrict__ pub65,
                                                       uint8_t* __restrict__ addr20, uint8_t* __restrict__ status) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    sc d;
    load32_be(d.v, seckey32 + (size_t)i * 32);
    const bool keyok = seckey_ok(d);
    sc_set_one_unless(d, keyok);
    gej9 P;
    bool pinf;  // d in [1, n): never the identity
    comb_mul_g9(P, pinf, d, gtab);
    fe px, py;
    gej9_to_affine_words(px, py, P);
    store_pub_addr(pub65 + (size_t)i * 65, addr20 ? addr20 + (size_t)i * 20 : nullptr, keyok, px, py);
    status[i] = keyok ? GSV_ST_OK : GSV_ST_INVALID_KEY;
}

// ---------------------------------------------------------------------------- launchers
hipError_t launch_ecsign(const uint8_t* msg32, const uint8_t* seckey32, uint32_t n, const uint4* gtab, uint8_t* sig65,
                         uint8_t* status, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ecsign, dim3((n + 255) / 256), dim3(256), 0, st, msg32, seckey32, n, gtab, sig65, status);
    return hipGetLastError();
}

hipError_t launch_pubkey_create(const uint8_t* seckey32, uint32_t n, const uint4* gtab, uint8_t* pub65,
                                uint8_t* addr20, uint8_t* status, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_pubkey_create, dim3((n + 255) / 256), dim3(256), 0, st, seckey32, n, gtab, pub65, addr20,
                       status);
    return hipGetLastError();
}

}  // namespace gsv

GSV_OPCOUNT_READER(ecsign)
