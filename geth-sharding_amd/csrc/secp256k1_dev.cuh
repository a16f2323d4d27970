// The numbers of the secp256k1 device code, in one place: the moduli, the generator, the GLV
// endomorphism's constants with its lattice, and the ladder's window.  Definitions only; the code
// that uses them is in secp256k1_scalar.cuh (words and scalars mod n), secp256k1_point.cuh and
// secp256k1_glv.cuh.  tests/secp_glv_model.py parses every one of them from this file's text
// (COMB_BITS from gsv_internal.h) and expects exactly one definition of each.
//
// 256-bit values are 8 x 32-bit little-endian limbs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsv {

// ------------------------------------------------------------------ the moduli
// p limbs (little endian)
__device__ constexpr uint32_t FP[8] = {0xFFFFFC2Fu, 0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu,
                                       0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};

// n limbs
__device__ constexpr uint32_t SN[8] = {0xD0364141u, 0xBFD25E8Cu, 0xAF48A03Bu, 0xBAAEDCE6u,
                                       0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
// 2^256 - n (129 bits)
__device__ constexpr uint32_t SNC[5] = {0x2FC9BEBFu, 0x402DA173u, 0x50B75FC4u, 0x45512319u, 1u};
// p - n: r + n is a field element for r below it (the x = r + n candidates of recovery and verification)
__device__ constexpr uint32_t P_MINUS_N[8] = {0x2FC9BAEEu, 0x402DA172u, 0x50B75FC4u, 0x45512319u,
                                              0x00000001u, 0u, 0u, 0u};
// (n - 1) / 2: a scalar above it is "high"
__device__ constexpr uint32_t HALF_N[8] = {0x681B20A0u, 0xDFE92F46u, 0x57A4501Du, 0x5D576E73u,
                                           0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x7FFFFFFFu};

// ------------------------------------------------------------------ the generator
__device__ constexpr uint32_t GX[8] = {0x16F81798u, 0x59F2815Bu, 0x2DCE28D9u, 0x029BFCDBu,
                                       0xCE870B07u, 0x55A06295u, 0xF9DCBBACu, 0x79BE667Eu};
__device__ constexpr uint32_t GY[8] = {0xFB10D4B8u, 0x9C47D08Fu, 0xA6855419u, 0xFD17B448u,
                                       0x0E1108A8u, 0x5DA4FBFCu, 0x26A3C465u, 0x483ADA77u};

// ------------------------------------------------------------------ the endomorphism (secp256k1_glv.cuh)
// lambda (x, y) = (beta x, y); the split k = r1 + r2 lambda (libsecp256k1 scalar_impl.h
// secp256k1_scalar_split_lambda) with c_i = round(k g_i / 2^272)
__device__ constexpr uint32_t BETA[8] = {0x719501EEu, 0xC1396C28u, 0x12F58995u, 0x9CF04975u,
                                         0xAC3434E9u, 0x6E64479Eu, 0x657C0710u, 0x7AE96A2Bu};
__device__ constexpr uint32_t MINUS_LAMBDA[8] = {0xB51283CFu, 0xE0CFC810u, 0x8EC739C2u, 0xA880B9FCu,
                                                 0x77ED9BA4u, 0x5AD9E3FDu, 0x3FA3CF1Fu, 0xAC9C52B3u};
__device__ constexpr uint32_t MINUS_B1[8] = {0x0ABFE4C3u, 0x6F547FA9u, 0x010E8828u, 0xE4437ED6u,
                                             0u, 0u, 0u, 0u};
// -b2 mod n: what libsecp256k1's split multiplies by (tests/secp_glv_model.py reads it); the device
// multiplies by b2 = n - MINUS_B2 (GLV_B2 at sc_split_lambda) and subtracts
__device__ constexpr uint32_t MINUS_B2[8] = {0x3DB1562Cu, 0xD765CDA8u, 0x0774346Du, 0x8A280AC5u,
                                             0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
__device__ constexpr uint32_t GLV_G1[8] = {0xEB153DABu, 0x90E49284u, 0x6BCDE86Cu, 0xD221A7D4u,
                                           0x00003086u, 0u, 0u, 0u};
__device__ constexpr uint32_t GLV_G2[8] = {0xE4C42212u, 0x7FA90ABFu, 0x88286F54u, 0x7ED6010Eu,
                                           0x0000E443u, 0u, 0u, 0u};
__device__ constexpr uint32_t GLV_B2[4] = {0x9284EB15u, 0xE86C90E4u, 0xA7D46BCDu, 0x3086D221u};
// vectors of the GLV lattice {(a, b) : a + b lambda == 0 mod n} (libsecp256k1 scalar_impl.h's basis)
// that glv_make_odd adds: v1 = (V1A, V1B) = (a1, b1), v2 = (V2A, V1A) = (a2, a1), v1 + v2 = (V3A, V3B)
__device__ constexpr uint32_t GLV_V1A[8] = {0x9284EB15u, 0xE86C90E4u, 0xA7D46BCDu, 0x3086D221u, 0u, 0u, 0u, 0u};
__device__ constexpr uint32_t GLV_V1B[8] = {0xC5765C7Eu, 0x507DDEE3u, 0xAE3A1813u, 0xD66B5E10u,
                                            0xFFFFFFFDu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
__device__ constexpr uint32_t GLV_V2A[8] = {0x9D44CFD8u, 0x57C1108Du, 0xA8E2F3F6u, 0x14CA50F7u, 1u, 0u, 0u, 0u};
__device__ constexpr uint32_t GLV_V3A[8] = {0x2FC9BAEDu, 0x402DA172u, 0x50B75FC4u, 0x45512319u, 1u, 0u, 0u, 0u};
__device__ constexpr uint32_t GLV_V3B[8] = {0x57FB4793u, 0x38EA6FC8u, 0x560E83E1u, 0x06F23032u,
                                            0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};

// ------------------------------------------------------------------ the ladder's window (secp256k1_glv.cuh)
// The GLV halves are recoded into fixed-schedule odd digits of GLV_W bits: digits in
// {+-1, +-3, ..., +-(2^W - 1)}, a table of the 2^(W-1) odd multiples of the point, W doublings per
// digit.  (w = 5 measured slower, r02-r05: DESIGN.md §7.3)
constexpr int GLV_W = 4;
constexpr int GLV_NT = 1 << (GLV_W - 1);             // table entries
constexpr int GLV_DIGITS = (130 + GLV_W - 1) / GLV_W;  // |k| < 2^130: the split gives < 2^128, + a lattice vector (glv_make_odd) < 2^129.3

}  // namespace gsv
