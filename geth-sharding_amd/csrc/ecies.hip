// Batched ecies.Encrypt / PrivateKey.Decrypt for ECIES_AES128_SHA256 on gfx950 (crypto/ecies/ecies.go:
// 246-366, s1 empty) — one item per lane, around the existing ladder (ecdh.hip):
//
//   Decrypt   k_ecies_parse    the checks on the ciphertext's shape, R and the secret key, in the
//                              reference's order (include/gsv.h numbers them); gathers R into a row
//             k_ecdh           Ke || Km of (R, secret key)                          [ecdh.hip, untouched]
//             k_ecies_open     tag check and AES-128-CTR in one pass (ecies_sym_dev.cuh); zeroes what it
//                              wrote when the tag fails; final status, msg_len, the slot's tail
//   Encrypt   k_pubkey_create  R = eph G                                            [ecsign.hip, untouched]
//             k_ecdh           Ke || Km of (recipient, eph)
//             k_ecies_seal     04 || R || iv || CTR || tag, or zeros
//
// The launches of one call share the caller's work area (`work`, no padding between its parts):
//   Decrypt   keys48[48 n] | R as X || Y [64 n] | the ladder's status [n]                    113 n bytes
//   Encrypt   keys48[48 n] | R as 04 || X || Y [65 n] | the ladder's status [n] | k_pubkey_create's [n]
// and the last kernel of a call overwrites its item's part of every region with zeros.
#include "opcount.cuh"
#include "gsv_internal.h"
#include "secp256k1_scalar.cuh"
#include "secp256k1_fe9.cuh"
#include "secp256k1_point.cuh"
#include "ecies_sym_dev.cuh"

namespace gsv {

GSV_DI uint32_t load_be32(const uint8_t* p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}
GSV_DI void store_be32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}
GSV_DI void zero_bytes(uint8_t* p, uint32_t from, uint32_t to) {
    for (uint32_t j = from; j < to; j++) p[j] = 0;
}

// ---------------------------------------------------------------------------- Decrypt, before the ladder
// status: checks 1-8 of include/gsv.h (the first failure decides).  point64 row i: R's X || Y when the
// ciphertext has them (98 bytes or more under a first byte of 04), else zeros, which the ladder refuses.
__global__ __launch_bounds__(256) void k_ecies_parse(const uint8_t* __restrict__ ct, const uint64_t* __restrict__ ct_off,
                                                     const uint8_t* __restrict__ seckey32, uint32_t n,
                                                     uint8_t* __restrict__ point64, uint8_t* __restrict__ status) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t off = ct_off[i], len = ct_off[i + 1] - off;
    const uint8_t* c = ct + off;
    uint32_t st = GSV_ST_OK;
    if (len == 0) {
        st = GSV_ST_INVALID_MESSAGE;
    } else {
        const uint32_t b0 = c[0];
        if (b0 < 2u || b0 > 4u) st = GSV_ST_INVALID_PUBKEY;
        else if (len < 98) st = GSV_ST_INVALID_MESSAGE;  // rLen + hLen + 1, rLen = 65 for 02, 03 and 04
        else if (b0 != 4u) st = GSV_ST_INVALID_PUBKEY;   // elliptic.Unmarshal takes only 04 || X || Y
    }
    uint32_t xw[8], yw[8], k[8];
#pragma unroll
    for (int j = 0; j < 8; j++) xw[j] = yw[j] = 0u;
    if (st == GSV_ST_OK) {
        load32_be(xw, c + 1);
        load32_be(yw, c + 33);
    }
    load32_be(k, seckey32 + (size_t)i * 32);
    // 5. a coordinate >= p is refused (the strict reading of elliptic.Unmarshal)
    if (st == GSV_ST_OK && !(limbs_lt(xw, FP) && limbs_lt(yw, FP))) st = GSV_ST_INVALID_PUBKEY;
    // 6. IsOnCurve (ecies.go:337), as k_ecdh tests it
    fe9 px, py;
    fe9_from_words(px, xw);
    fe9_from_words(py, yw);
    fe9_normalize_full(px);
    fe9_normalize_full(py);
    const bool curve_ok = on_curve9(px, py);  // every lane computes it
    if (st == GSV_ST_OK && !curve_ok) st = GSV_ST_INVALID_CURVE;
    // 7. the secret key in [1, n) (seckey_ok's verdict; its OR-reduction in place of this chain of
    // compares changes the kernel's instructions, so the chain stays)
    bool kzero = true;
#pragma unroll
    for (int j = 0; j < 8; j++) kzero = kzero && k[j] == 0u;
    if (st == GSV_ST_OK && (kzero || !limbs_lt(k, SN))) st = GSV_ST_INVALID_KEY;
    // 8. em shorter than an IV
    if (st == GSV_ST_OK && len < GSV_ECIES_OVERHEAD) st = GSV_ST_INVALID_MESSAGE;
    limbs_to_be(point64 + (size_t)i * 64, xw);
    limbs_to_be(point64 + (size_t)i * 64 + 32, yw);
    status[i] = (uint8_t)st;
}

// the byte range of item i's s2, empty without a table
GSV_DI const uint8_t* s2_of(const uint8_t* s2, const uint64_t* s2_off, uint32_t i, uint32_t& len) {
    len = 0;
    if (!s2_off) return s2;
    len = (uint32_t)(s2_off[i + 1] - s2_off[i]);
    return s2 + s2_off[i];
}

// ---------------------------------------------------------------------------- Decrypt, behind the ladder
// status in: k_ecies_parse's; out: the final one.  Item i owns msg_out[ct_off[i] .. ct_off[i + 1]): the
// message, then zeros; all zeros when it failed.
__global__ __launch_bounds__(256) void k_ecies_open(const uint8_t* __restrict__ ct, const uint64_t* __restrict__ ct_off,
                                                    const uint8_t* __restrict__ s2, const uint64_t* __restrict__ s2_off,
                                                    uint32_t n, uint8_t* __restrict__ work, uint8_t* __restrict__ msg_out,
                                                    uint32_t* __restrict__ msg_len, uint8_t* __restrict__ status) {
    __shared__ uint32_t te[AES_TE0_WORDS];
    aes_te0_fill(te, threadIdx.x);
    __syncthreads();
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint8_t* keys = work + (size_t)i * 48;
    uint8_t* row = work + (size_t)n * 48 + (size_t)i * 64;
    uint8_t* est = work + (size_t)n * 112 + i;
    const uint64_t off = ct_off[i];
    const uint32_t len = (uint32_t)(ct_off[i + 1] - off);
    const uint8_t* c = ct + off;
    uint8_t* o = msg_out + off;
    uint32_t st = status[i];
    if (st == GSV_ST_OK && *est != GSV_ST_OK) st = *est;  // the ladder's own verdict (k P = O: cannot happen)
    if (st == GSV_ST_OK) {  // len >= 113
        uint32_t ke[4], km[8], iv[4], tag[8];
#pragma unroll
        for (int j = 0; j < 4; j++) ke[j] = load_be32(keys + 4 * j);
#pragma unroll
        for (int j = 0; j < 8; j++) km[j] = load_be32(keys + 16 + 4 * j);
#pragma unroll
        for (int j = 0; j < 4; j++) iv[j] = load_be32(c + 65 + 4 * j);
        uint32_t s2len;
        const uint8_t* s2p = s2_of(s2, s2_off, i, s2len);
        ecies_sym<false>(tag, ke, km, c + 81, len - GSV_ECIES_OVERHEAD, iv, s2p, s2len, o, te);
        // subtle.ConstantTimeCompare: no early exit
        uint32_t diff = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) diff |= tag[j] ^ load_be32(c + len - 32 + 4 * j);
        if (diff) st = GSV_ST_INVALID_MESSAGE;
    }
    const uint32_t mlen = st == GSV_ST_OK ? len - GSV_ECIES_OVERHEAD : 0u;
    zero_bytes(o, mlen, len);  // the slot's tail; the whole slot, the plaintext just written included, when it failed
    status[i] = (uint8_t)st;
    msg_len[i] = mlen;
    zero_bytes(keys, 0, 48);
    zero_bytes(row, 0, 64);
    *est = 0;
}

// ---------------------------------------------------------------------------- Encrypt, behind the ladder
// Item i is written at ct_out + msg_off[i] + 113 i: 113 + len(m) bytes, zeros when it failed.
__global__ __launch_bounds__(256) void k_ecies_seal(const uint8_t* __restrict__ msg, const uint64_t* __restrict__ msg_off,
                                                    const uint8_t* __restrict__ iv16, const uint8_t* __restrict__ s2,
                                                    const uint64_t* __restrict__ s2_off, uint32_t n,
                                                    uint8_t* __restrict__ work, uint8_t* __restrict__ ct_out,
                                                    uint8_t* __restrict__ status) {
    __shared__ uint32_t te[AES_TE0_WORDS];
    aes_te0_fill(te, threadIdx.x);
    __syncthreads();
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint8_t* keys = work + (size_t)i * 48;
    uint8_t* row = work + (size_t)n * 48 + (size_t)i * 65;
    uint8_t* est = work + (size_t)n * 113 + i;
    uint8_t* pst = work + (size_t)n * 114 + i;
    const uint64_t off = msg_off[i];
    const uint32_t mlen = (uint32_t)(msg_off[i + 1] - off);
    uint8_t* o = ct_out + off + (size_t)GSV_ECIES_OVERHEAD * i;
    uint32_t st = *est;  // the key rule, then the curve rule
    if (st == GSV_ST_OK && *pst != GSV_ST_OK) st = *pst;
    if (st == GSV_ST_OK && mlen == 0u) st = GSV_ST_INVALID_MESSAGE;  // the reference returns (nil, nil)
    if (st == GSV_ST_OK) {
        uint32_t ke[4], km[8], iv[4], tag[8];
#pragma unroll
        for (int j = 0; j < 4; j++) ke[j] = load_be32(keys + 4 * j);
#pragma unroll
        for (int j = 0; j < 8; j++) km[j] = load_be32(keys + 16 + 4 * j);
#pragma unroll
        for (int j = 0; j < 4; j++) iv[j] = load_be32(iv16 + (size_t)i * 16 + 4 * j);
        for (int j = 0; j < 65; j++) o[j] = row[j];
#pragma unroll
        for (int j = 0; j < 4; j++) store_be32(o + 65 + 4 * j, iv[j]);
        uint32_t s2len;
        const uint8_t* s2p = s2_of(s2, s2_off, i, s2len);
        ecies_sym<true>(tag, ke, km, msg + off, mlen, iv, s2p, s2len, o + 81, te);
#pragma unroll
        for (int j = 0; j < 8; j++) store_be32(o + 81 + mlen + 4 * j, tag[j]);
    } else {
        zero_bytes(o, 0, GSV_ECIES_OVERHEAD + mlen);
    }
    status[i] = (uint8_t)st;
    zero_bytes(keys, 0, 48);
    zero_bytes(row, 0, 65);
    *est = 0;
    *pst = 0;
}

// ---------------------------------------------------------------------------- launchers
// 256-thread workgroups for n items, counted in 64 bits: n + 255 wraps in 32 for n near 2^32
static uint32_t blocks256(uint32_t n) { return (uint32_t)(((uint64_t)n + 255) / 256); }

hipError_t launch_ecies_parse(const uint8_t* ct, const uint64_t* ct_off, const uint8_t* seckey32, uint32_t n,
                              uint8_t* point64, uint8_t* status, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ecies_parse, dim3(blocks256(n)), dim3(256), 0, st, ct, ct_off, seckey32, n, point64, status);
    return hipGetLastError();
}

hipError_t launch_ecies_open(const uint8_t* ct, const uint64_t* ct_off, const uint8_t* s2, const uint64_t* s2_off,
                             uint32_t n, uint8_t* work, uint8_t* msg_out, uint32_t* msg_len, uint8_t* status,
                             hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ecies_open, dim3(blocks256(n)), dim3(256), 0, st, ct, ct_off, s2, s2_off, n, work, msg_out,
                       msg_len, status);
    return hipGetLastError();
}

hipError_t launch_ecies_seal(const uint8_t* msg, const uint64_t* msg_off, const uint8_t* iv16, const uint8_t* s2,
                             const uint64_t* s2_off, uint32_t n, uint8_t* work, uint8_t* ct_out, uint8_t* status,
                             hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ecies_seal, dim3(blocks256(n)), dim3(256), 0, st, msg, msg_off, iv16, s2, s2_off, n, work,
                       ct_out, status);
    return hipGetLastError();
}

}  // namespace gsv

GSV_OPCOUNT_READER(ecies)
