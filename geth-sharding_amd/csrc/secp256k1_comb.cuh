// u * G by the fixed-base comb over the context's table (gsv_internal.h COMB_BITS; built by
// ecrecover.hip k_gtable_base / k_gtable_init): recovery's and verification's u1 G, signing's k G and
// d G.  No doublings and no exceptional add, so nothing here reaches the rare-doubling hook.
#pragma once
#include "gsv_internal.h"
#include "secp256k1_scalar.cuh"
#include "secp256k1_fe9.cuh"

namespace gsv {

// comb table entry (w, d) = d * 2^(COMB_BITS w) * G, affine, canonical fe9 limbs: x[9] y[9] + 2 pad words
constexpr int GTAB_ENTRY_U4 = GTAB_ENTRY_BYTES / 16;
GSV_DI void gtab_load(ge9& P, const uint4* e) {
    uint4 a = e[0], b = e[1], c = e[2], d = e[3], f = e[4];
    uint32_t w[20] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w,
                      d.x, d.y, d.z, d.w, f.x, f.y, f.z, f.w};
#pragma unroll
    for (int i = 0; i < 9; i++) {
        P.x.v[i] = w[i];
        P.y.v[i] = w[9 + i];
    }
}

// the scalar shifted right by COMB_BITS in place (8 words; v_alignbit pairs)
GSV_DI void comb_shift(uint32_t c[8]) {
#pragma unroll
    for (int i = 0; i < 7; i++) c[i] = __builtin_amdgcn_alignbit(c[i + 1], c[i], COMB_BITS);
    c[7] >>= COMB_BITS;
}
// u*G with the fixed-base comb table (COMB_WINDOWS mixed adds, no doublings), summed in the W
// convention (the mixed add it shares with the GLV ladder) and returned Jacobian, Z magnitude 2.
// The windows' digits are
// read from the bottom of a copy of u shifted by COMB_BITS per window (r05): comb_digit's word select
// with a loop-variant index was turned into a private array written to scratch and read back by a
// dynamic offset twice per window (72 bytes of scratch stores per window, ~0.8 KB per recovery; r04's
// 0.78 GB of writes per 2^20-recovery launch).
GSV_DI void comb_mul_g9(gej9& acc, bool& inf, const sc& u, const uint4* __restrict__ gtab) {
    constexpr uint32_t MASK = (1u << COMB_BITS) - 1u;
    uint32_t c[8] = {u.v[0], u.v[1], u.v[2], u.v[3], u.v[4], u.v[5], u.v[6], u.v[7]};
    ge9 Pn;
    const uint32_t d0 = c[0] & MASK;
    gtab_load(Pn, gtab + (size_t)d0 * GTAB_ENTRY_U4);
    // window 0 starts the sum: its entry is the accumulator (Z = 1), no add
    acc.x = Pn.x;
    fe9_add(acc.y, Pn.y, Pn.y);  // W = 2y, 2
    fe9_set_u32(acc.z, 1);
    inf = d0 == 0;
    comb_shift(c);  // c = u >> (COMB_BITS w) at the top of window w
    const uint32_t d1 = c[0] & MASK;
    gtab_load(Pn, gtab + (((size_t)1 << COMB_BITS) + d1) * GTAB_ENTRY_U4);
    // No add of the comb doubles or cancels (before window w the sum is
    // (u mod 2^(COMB_BITS w)) G, below the addend d 2^(COMB_BITS w) G, and the two together stay at or
    // below u < n), so none tests H: gejw_add_ge_z1 / gejw_add_ge_nx.  What does occur is the identity
    // start: low windows of u that are zero carry inf, and the addend becomes the accumulator.
    // Window 1 adds to window 0's entry, still affine (Z = 1).
    {
        ge9 P = Pn;
        if (COMB_WINDOWS > 2) {
            comb_shift(c);
            gtab_load(Pn, gtab + (((size_t)2 << COMB_BITS) + (c[0] & MASK)) * GTAB_ENTRY_U4);
        }
        gej9 t;
        gejw_add_ge_z1(t, acc, P);
        if (FE9_ANY(inf)) {
            gej9 qn;
            gejw_from_ge(qn, P);
            gej9_cmov(t, qn, inf);
        }
        if (d1 != 0) {
            acc = t;
            inf = false;
        }
    }
#pragma unroll 1
    for (int w = 2; w < COMB_WINDOWS; w++) {
        uint32_t d = c[0] & MASK;
        ge9 P = Pn;
        if (w < COMB_WINDOWS - 1) {  // prefetch next window's entry
            comb_shift(c);
            gtab_load(Pn, gtab + (((size_t)(w + 1) << COMB_BITS) + (c[0] & MASK)) * GTAB_ENTRY_U4);
        }
        gej9 t;
        bool tinf = inf;
        gejw_add_ge_nx(t, tinf, acc, P);
        if (d != 0) {
            acc = t;
            inf = tinf;
        }
    }
    gejw_to_gej9(acc, acc);
}

}  // namespace gsv
