// Inverses mod n of a group of recovery r values from ONE safegcd inversion (Montgomery's trick):
// prefix products forward, one modinv30_words of the whole product, back-substitution.  3 (k - 1)
// sc_mul and one inversion for k values; a sc_mul is about 1/20 of the inversion.  k_rinv_batch
// (ecrecover.hip) runs it with one group per lane ahead of k_ecrecover, which then loads r^-1 instead
// of inverting: a wave pays the slowest lane's divstep count, so what counts is how few waves invert.
//
// Host-compilable (tests/native/rinv_host.cpp, tests/test_rinv_batch.py): the device build takes sc
// and sc_mul from secp256k1_scalar.cuh (inline asm); without __HIPCC__ a plain C++ sc_mul stands in.
#pragma once
#include <stdint.h>

#include "modinv30.cuh"

#if defined(__HIPCC__)
#include "secp256k1_scalar.cuh"
#define RINV_FN __device__ __forceinline__
#else
#define RINV_FN static inline
namespace gsv {
struct sc { uint32_t v[8]; };
static constexpr uint32_t SN[8] = {0xD0364141u, 0xBFD25E8Cu, 0xAF48A03Bu, 0xBAAEDCE6u,
                                   0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
// a * b mod n, schoolbook: the 512-bit product, then 2^256 == 2^256 - n folded until the high half is
// empty (each fold shrinks it by 127 bits), then at most one subtraction of n
static inline void sc_mul(sc& r, const sc& a, const sc& b) {
    static constexpr uint32_t C[5] = {0x2FC9BEBFu, 0x402DA173u, 0x50B75FC4u, 0x45512319u, 1u};
    uint32_t t[24] = {0};
    for (int i = 0; i < 8; i++) {
        uint64_t c = 0;
        for (int j = 0; j < 8; j++) {
            c += (uint64_t)a.v[i] * b.v[j] + t[i + j];
            t[i + j] = (uint32_t)c;
            c >>= 32;
        }
        t[i + 8] = (uint32_t)c;
    }
    for (;;) {
        bool hi = false;
        for (int i = 8; i < 24; i++) hi = hi || t[i] != 0;
        if (!hi) break;
        uint32_t h[16], u[24] = {0};
        for (int i = 0; i < 16; i++) h[i] = t[8 + i];
        for (int i = 0; i < 8; i++) u[i] = t[i];
        for (int i = 0; i < 16; i++) {
            uint64_t c = 0;
            for (int j = 0; j < 5 && i + j < 24; j++) {
                c += (uint64_t)h[i] * C[j] + u[i + j];
                u[i + j] = (uint32_t)c;
                c >>= 32;
            }
            for (int k = i + 5; c != 0 && k < 24; k++) {
                c += u[k];
                u[k] = (uint32_t)c;
                c >>= 32;
            }
        }
        for (int i = 0; i < 24; i++) t[i] = u[i];
    }
    int64_t br = 0;
    uint32_t d[8];
    for (int i = 0; i < 8; i++) {
        int64_t x = (int64_t)t[i] - SN[i] + br;
        d[i] = (uint32_t)x;
        br = x >> 32;
    }
    for (int i = 0; i < 8; i++) r.v[i] = br ? t[i] : d[i];
}
}  // namespace gsv
#endif

namespace gsv {

// what enters the product for an r as read: r itself, or 1 where r == 0 or r >= n.  Such an item fails
// recovery through recover_core's own range checks and its inverse is never used; 1 keeps the other
// members' product invertible.
RINV_FN void sc_rinv_operand(sc& x) {
    uint32_t nz = 0;
    int64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        nz |= x.v[i];
        br = ((int64_t)x.v[i] - (int64_t)SN[i] + br) >> 32;
    }
    bool ok = nz != 0 && br != 0;  // 0 < x < n
#pragma unroll
    for (int i = 0; i < 8; i++) x.v[i] = ok ? x.v[i] : (i == 0 ? 1u : 0u);
}

// Slots: get(i, x) reads value i (any 256-bit number) in the form it is stored in and value(x) turns
// that form into limbs, so that a read issued a step ahead is waited for only where it is used;
// put(i, x) / take(i, x) write and read working slot i, which holds prefix product i between the two
// sweeps and value i's inverse, fully reduced, at the end.  cnt >= 1.  Few values are live at a time:
// the running product, two operands and the inversion's own state.
template <class Slots>
RINV_FN void sc_batch_inverse(Slots& sl, uint32_t cnt) {
    // each sweep reads the next step's operands before the products of this one: a lane's loads are
    // otherwise waited for in full, once a step (one wave per SIMD has nothing else to run)
    sc acc, x;
    sl.get(0, acc);
    sl.value(acc);
    sc_rinv_operand(acc);
    if (cnt > 1) sl.get(1, x);
    for (uint32_t i = 1; i < cnt; i++) {
        sc nx = x;
        sl.put(i, acc);  // r_0 ... r_(i-1)
        if (i + 1 < cnt) sl.get(i + 1, nx);
        sl.value(x);
        sc_rinv_operand(x);
        sc_mul(acc, acc, x);
        x = nx;
    }
    sc inv, p = acc;
    if (cnt > 1) sl.take(cnt - 1, p);  // x is r_(cnt-1) as read
    modinv30_words(inv.v, acc.v, MI30_N);  // (r_0 ... r_(cnt-1))^-1
    for (uint32_t i = cnt - 1; i >= 1; i--) {
        sc np = p, nx = x;
        if (i > 1) {
            sl.take(i - 1, np);
            sl.get(i - 1, nx);
        }
        sl.value(x);
        sc_rinv_operand(x);
        sc_mul(p, p, inv);  // r_i^-1
        sl.put(i, p);
        sc_mul(inv, inv, x);  // (r_0 ... r_(i-1))^-1
        p = np;
        x = nx;
    }
    sl.put(0, inv);
}

}  // namespace gsv
