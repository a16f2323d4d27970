// The GLV scalar multiplication k * P of the secp256k1 kernels (recovery's u2 R on its twist,
// verification's u2 P, ECDH's k P): the lambda split, the lattice step that makes both halves odd,
// and the w = 4 fixed-schedule ladder over a per-lane table in LDS.  ecrecover.hip tells the whole
// algorithm; glv_sched.cuh holds the integer-only pieces that also build for the host.
//
// INCLUDE ORDER: this header comes before any other that includes secp256k1_fe9.cuh.  It routes the
// mixed adds' rare p == q doubling to an out-of-line function through the field header's
// GEJ9_DBL_RARE / GEJW_DBL_RARE hook (secp256k1_fe9.cuh says why), which has to be set before that
// header is first read.  Getting it wrong is a compile error, below.
#pragma once
#include "secp256k1_scalar.cuh"
namespace gsv {
struct gej9;
__device__ void gej9_dbl_rare(gej9& o, const gej9& p);
__device__ void gejw_dbl_rare(gej9& o, const gej9& p);
}
#define GEJ9_DBL_RARE(o, p) gej9_dbl_rare(o, p)
#define GEJW_DBL_RARE(o, p) gejw_dbl_rare(o, p)
#include "secp256k1_fe9.cuh"
#if defined(FE9_GEJ9_DBL_RARE_INLINE) || defined(FE9_GEJW_DBL_RARE_INLINE)
#error "secp256k1_fe9.cuh was included before secp256k1_glv.cuh: the ladder's mixed adds would get the inline doubling. Include secp256k1_glv.cuh first."
#endif
#include "secp256k1_point.cuh"
#include "glv_sched.cuh"

namespace gsv {

// GLV_W, GLV_NT, GLV_DIGITS and the endomorphism's constants: secp256k1_dev.cuh
// the ladder's doubling returns -2P (gejw_dbl_neg): the sign is back to + after an even run
static_assert(GLV_W % 2 == 0, "an odd run of negating doublings leaves the accumulator at -2^W P");
// digit code = sign bit above a (W - 1)-bit table index, packed in DIG_SLOT-bit slots
constexpr int DIG_SLOT = GLV_W <= 4 ? 4 : 8;
constexpr int DIG_PER_WORD = 32 / DIG_SLOT;
constexpr int DIG_WORDS = (GLV_DIGITS + DIG_PER_WORD - 1) / DIG_PER_WORD;
static_assert(GLV_W >= 3 && GLV_W <= 5, "GLV window width");
// where the per-lane GLV table lives: entries 0..3 in LDS ([word][256 lanes] per block), the rest in a
// private array (scratch: memory only for resident lanes, served by L1/L2).  Two waves per SIMD leave
// LDS room for 72 words a lane: four entries.  (The whole table private measured 107.2 vs 113.7-114.3 M
// recoveries/s, r05: profiles/r05/ab/ecrecover_options.txt.)
constexpr int GLV_LNT = 4;  // entries in LDS
static_assert(GLV_LNT <= GLV_NT, "LDS holds at most four entries at two waves per SIMD");
// LDS part: 18 GLV_LNT words per lane, lane-minor ([word][GSV_LTAB_STRIDE]); the kernels that call
// glv_mul_point (through recover_core or verify_core) run 256-thread blocks and declare
// __shared__ uint32_t[GSV_LTAB_WORDS].
constexpr int GSV_LTAB_STRIDE = 256;
constexpr int GSV_LTAB_WORDS = 18 * GLV_LNT * GSV_LTAB_STRIDE;
// Measured and not kept (r02-r05): the lambda half's x coordinates (beta x_e) precomputed per entry in
// a private array (+0.3 %, but 4.6x the fetch bytes: profiles/r02/ab_betatab.txt), the private half
// read one add ahead (112.3-112.8 vs 113.7-114.3 M/s) and the two adds of a digit position as
// straight-line code (equal) (profiles/r05/ab/ecrecover_options.txt).
#define GSV_LTAB_DECL __shared__ uint32_t ltab[GSV_LTAB_WORDS]
#define GSV_LTAB_LANE (ltab + threadIdx.x)

// ---------------------------------------------------------------------------- the split
// (k * g) >> 272, rounded (libsecp256k1 scalar_8x32_impl.h mul_shift_var semantics)
GSV_DI void sc_mul_shift272(sc& r, const sc& k, const uint32_t g[8]) {
    GSV_OPC(OPC_SC_MUL);
    uint32_t t[16];
    mul_8x8_fx(t, k.v, g);
#pragma unroll
    for (int i = 0; i < 7; i++) r.v[i] = (t[8 + i] >> 16) | (t[9 + i] << 16);
    r.v[7] = t[15] >> 16;
    uint64_t c = (uint64_t)r.v[0] + ((t[8] >> 15) & 1u);
    r.v[0] = lo32(c);
#pragma unroll
    for (int i = 1; i < 8; i++) {
        c = (uint64_t)r.v[i] + hi32(c);
        r.v[i] = lo32(c);
    }
}

// k = r1 + r2 * lambda (mod n)  (libsecp256k1 scalar_impl.h secp256k1_scalar_split_lambda):
// r2 = c1 (-b1) + c2 (-b2), r1 = k - r2 lambda, with c_i = round(k g_i / 2^272).
// The two products of r2 are short.  k < 2^256, so c_i <= (2^256 g_i) / 2^272 + 1 = g_i / 2^16 + 1:
// g1 < 2^142 gives c1 < 2^126, g2 < 2^144 with g2 >> 16 = 0xE4437ED6...E4C4 gives c2 < 2^128.
// -b1 = MINUS_B1 < 2^128 and b2 = n - MINUS_B2 = GLV_B2 < 2^126 (it is the lattice's a1, GLV_V1A).
// So c1 (-b1) < 2^254 and c2 b2 < 2^254 are 4 x 4-limb products, both below n: no reduction, and
// r2 = c1 (-b1) - c2 b2 + (n if that is negative) is the same residue sc_mul and sc_add gave
// (c2 (-b2) = c2 n - c2 b2).  tests/test_secp_recover_trim.py asserts the four bounds on the model's
// boundary scalars.  (Not counted as OPC_SC_MUL: tools/count_ops.py reads two scalar products fewer.)
GSV_DI void sc_split_lambda(sc& r1, sc& r2, const sc& k) {
    sc c1, c2, t;
    sc_mul_shift272(c1, k, GLV_G1);
    sc_mul_shift272(c2, k, GLV_G2);
    const uint32_t nb1[4] = {MINUS_B1[0], MINUS_B1[1], MINUS_B1[2], MINUS_B1[3]};
    const uint32_t b2[4] = {GLV_B2[0], GLV_B2[1], GLV_B2[2], GLV_B2[3]};
    uint32_t n[8];
#pragma unroll
    for (int i = 0; i < 8; i++) n[i] = SN[i];
    glv_short_r2(r2.v, c1.v, nb1, c2.v, b2, n);
    sc_from_const(t, MINUS_LAMBDA);
    sc_mul(r1, r2, t);
    sc_add(r1, r1, k);
}

// The ladder's digits are read from the scalar's bits where they are used (glv_sched.cuh says why
// that is the fixed-schedule odd-digit recoding): K = k >> 1 in DIG_WORDS words, digit i in slot i.
static_assert(DIG_SLOT == GLV_W, "the digits are read in place: slot i of the halved scalar is K_i");

// ---------------------------------------------------------------------------- the rare doubling
// Doubling for the rare p == q case of the mixed add, out of line so the hot loops stay small
// in I-cache; the point travels in VGPR vectors (an aggregate or pointer argument would pin the
// caller's accumulator to scratch memory).
typedef uint32_t gsv_v32 __attribute__((ext_vector_type(32)));
template <bool WCONV>
__device__ __noinline__ gsv_v32 gej9_dbl_ool(gsv_v32 in) {
    gej9 p, d;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        p.x.v[i] = in[i];
        p.y.v[i] = in[9 + i];
        p.z.v[i] = in[18 + i];
    }
    if (WCONV) gejw_dbl(d, p);
    else gej9_dbl(d, p);
    gsv_v32 o;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        o[i] = d.x.v[i];
        o[9 + i] = d.y.v[i];
        o[18 + i] = d.z.v[i];
    }
#pragma unroll
    for (int i = 27; i < 32; i++) o[i] = 0;
    return o;
}
template <bool WCONV>
GSV_DI void gej9_dbl_rare_call(gej9& o, const gej9& p) {
    gsv_v32 in;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        in[i] = p.x.v[i];
        in[9 + i] = p.y.v[i];
        in[18 + i] = p.z.v[i];
    }
#pragma unroll
    for (int i = 27; i < 32; i++) in[i] = 0;
    gsv_v32 d = gej9_dbl_ool<WCONV>(in);
#pragma unroll
    for (int i = 0; i < 9; i++) {
        o.x.v[i] = d[i];
        o.y.v[i] = d[9 + i];
        o.z.v[i] = d[18 + i];
    }
}
__device__ void gej9_dbl_rare(gej9& o, const gej9& p) { gej9_dbl_rare_call<false>(o, p); }
__device__ void gejw_dbl_rare(gej9& o, const gej9& p) { gej9_dbl_rare_call<true>(o, p); }

// ---------------------------------------------------------------------------- the lattice step
// Both GLV halves are made odd before the recoding by adding a vector of the GLV lattice
// ({(a, b) : a + b lambda == 0 mod n}, libsecp256k1 scalar_impl.h's basis), so the odd-digit recoding
// needs no skew and the two skew-correcting mixed adds at the end of u2 R disappear.  v1 = (a1, b1)
// has odd/odd coordinates, v2 = (a2, a1) even/odd, v1 + v2 odd/even: one of them (or none) turns the
// magnitudes |k1|, |k2| (parity of k mod n XOR its sign, n being odd) both odd.  |a1| < 2^126,
// |b1| < 2^128, |a2| < 2^129: |k| < 2^128 grows below 2^129.3 < 2^130, inside GLV_DIGITS' range.
GSV_DI void glv_make_odd(sc& k1, sc& k2) {
    bool odd1 = ((k1.v[0] & 1u) != 0) != sc_is_high(k1);  // parity of |k1|
    bool odd2 = ((k2.v[0] & 1u) != 0) != sc_is_high(k2);
    // (flip k1, flip k2): (1, 1) v1, (0, 1) v2 = (a2, a1), (1, 0) v1 + v2, (0, 0) nothing
    bool use1 = !odd1 && !odd2, use2 = odd1 && !odd2, use3 = !odd1 && odd2;
    sc A, B;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        A.v[i] = use1 ? GLV_V1A[i] : use2 ? GLV_V2A[i] : use3 ? GLV_V3A[i] : 0u;
        B.v[i] = use1 ? GLV_V1B[i] : use2 ? GLV_V1A[i] : use3 ? GLV_V3B[i] : 0u;
    }
    sc_add(k1, k1, A);
    sc_add(k2, k2, B);
}

// ---------------------------------------------------------------------------- u2 * P
// out = u2 * (x, y) via GLV + fixed w = GLV_W odd digits, Jacobian (X, Y, Z magnitude 1);
// outinf: the ladder ended at the identity.  (x, y), magnitude 1, is a point of order n on any curve
// y^2 = x^3 + b: recovery's R on its twist (recover_core), verification's parsed key on E
// (ecverify.hip).  ltab: this lane's column of the block's LDS table (GSV_LTAB_LANE).
GSV_DI void glv_mul_point(gej9& out, bool& outinf, const sc& u2, const fe9& x, const fe9& y,
                          uint32_t* __restrict__ ltab) {
    sc k1, k2;
    sc_split_lambda(k1, k2, u2);
    glv_make_odd(k1, k2);  // both halves odd: the recoding's skews are 0, no correcting adds
    bool neg1 = sc_is_high(k1), neg2 = sc_is_high(k2);
    {
        sc nk;
        sc_neg(nk, k1);
#pragma unroll
        for (int i = 0; i < 8; i++) k1.v[i] = neg1 ? nk.v[i] : k1.v[i];
        sc_neg(nk, k2);
#pragma unroll
        for (int i = 0; i < 8; i++) k2.v[i] = neg2 ? nk.v[i] : k2.v[i];
    }
    uint32_t K1[DIG_WORDS], K2[DIG_WORDS];  // the halved magnitudes: digit i sits in slot i
    glv_halve(K1, k1.v);
    glv_halve(K2, k2.v);

    // The GLV table {x[GLV_NT], y[GLV_NT]} of the odd multiples (2e+1)R lives in LDS (w = 3:
    // ltab = this lane's column of a [word][256 lanes] array, conflict-free for any per-lane entry
    // index) or in a private array (wider windows), not in VGPRs, which would cost occupancy.
    // Each add loads its entry by index (no selects); lambda(P) = (beta x, y) costs one product per
    // lambda add.
    // entry e < GLV_LNT: LDS words [e*9 + k] (x) and [9*GLV_LNT + e*9 + k] (y); the others: the
    // private array, x at [(e - GLV_LNT)*9 + k], y after all x
    constexpr int PNT = GLV_NT - GLV_LNT;
    uint32_t ptab[18 * (PNT > 0 ? PNT : 1)];
#define GLV_L(i) ltab[(i) * GSV_LTAB_STRIDE]
#define GLV_X(e, k) ((e) < GLV_LNT ? GLV_L((e) * 9 + (k)) : ptab[((e) - GLV_LNT) * 9 + (k)])
#define GLV_Y(e, k) ((e) < GLV_LNT ? GLV_L(9 * GLV_LNT + (e) * 9 + (k)) : ptab[9 * PNT + ((e) - GLV_LNT) * 9 + (k)])
#define GLV_SET(e, k, X, Y)                                           \
    do {                                                              \
        if ((e) < GLV_LNT) {                                          \
            GLV_L((e) * 9 + (k)) = (X);                               \
            GLV_L(9 * GLV_LNT + (e) * 9 + (k)) = (Y);                 \
        } else {                                                      \
            ptab[((e) - GLV_LNT) * 9 + (k)] = (X);                    \
            ptab[9 * PNT + ((e) - GLV_LNT) * 9 + (k)] = (Y);          \
        }                                                             \
    } while (0)
    // Odd multiples on an isomorphic curve E'' (affine there, no inversion): P_e = (2e+1)R' built
    // by mixed adds of D = 2R' with their z-ratios zr_e, stored unscaled, then every entry below the
    // last rescaled to the last one's Z by the product of the later z-ratios.  A Jacobian result
    // (X, Y, Z) on E'' is (X, Y, Z zfac) on E.
    // Built with co-Z arithmetic (secp256k1_fe9.cuh ge9_dblu / ge9_zaddu): the pair (2R, R) at the
    // common Z = 2y, then each P_e = D + P_{e-1} keeps D co-Z with it; z-ratios as above.
    fe9 zfac;
    {
        ge9 Dp, P;
        fe9 zd;
        ge9_dblu(Dp, P, zd, x, y);
        fe9 zr[GLV_NT];
#pragma unroll
        for (int e = 0; e < GLV_NT; e++) {
            if (e) {
                ge9 Pn;
                ge9_zaddu(Pn, Dp, zr[e], P);
                P = Pn;
            }
#pragma unroll
            for (int k = 0; k < 9; k++) GLV_SET(e, k, P.x.v[k], P.y.v[k]);
        }
        fe9 f = zr[GLV_NT - 1];
#pragma unroll
        for (int e = GLV_NT - 2; e >= 0; e--) {
            fe9 ex, ey;
#pragma unroll
            for (int k = 0; k < 9; k++) {
                ex.v[k] = GLV_X(e, k);
                ey.v[k] = GLV_Y(e, k);
            }
            ge9 q;
            scale_xy9(q, ex, ey, f);
#pragma unroll
            for (int k = 0; k < 9; k++) GLV_SET(e, k, q.x.v[k], q.y.v[k]);
            if (e) fe9_mul(f, f, zr[e]);  // 1
        }
        fe9_mul(zfac, f, zd);  // f = all the z-ratios: the entries' common Z on E is zd f
    }

    // One entry of the table for the add of pass j (0: T, 1: lambda(T) = (beta x, y)), negated where
    // the digit's sign and the half's sign differ: x, y magnitude <= 1, <= 2.  (A macro, not a lambda: a
    // captured ptab turns both halves of the table into flat loads through 64-bit addresses.)
#define GLV_ENTRY(P, ei, negate, j)                                                                    \
    do {                                                                                               \
        if (GLV_LNT == GLV_NT || (GLV_LNT > 0 && (ei) < (uint32_t)GLV_LNT)) {                          \
            uint32_t xo = (ei) * 9u;                                                                   \
            _Pragma("unroll") for (int k = 0; k < 9; k++) {                                            \
                P.x.v[k] = GLV_L(xo + k);                                                              \
                P.y.v[k] = GLV_L(9u * GLV_LNT + xo + k);                                               \
            }                                                                                          \
        } else { /* the lanes whose digit indexes the private part (divergent: each side loads only its lanes) */ \
            uint32_t xo = ((ei) - (uint32_t)GLV_LNT) * 9u;                                             \
            _Pragma("unroll") for (int k = 0; k < 9; k++) {                                            \
                P.x.v[k] = ptab[xo + k];                                                               \
                P.y.v[k] = ptab[9u * PNT + xo + k];                                                    \
            }                                                                                          \
        }                                                                                              \
        if ((j) != 0) { /* wave-uniform */                                                             \
            fe9 beta;                                                                                  \
            fe9_from_const(beta, BETA);                                                                \
            fe9_mul(P.x, P.x, beta);                                                                   \
        }                                                                                              \
        fe9 ny;                                                                                        \
        fe9_neg<1>(ny, P.y); /* 2 */                                                                   \
        fe9_cmov(P.y, ny, (negate));                                                                   \
    } while (0)
    gej9 acc;  // W convention (X, 2Y, Z) through the ladder
    // The top digits (positive, index K >> w (GLV_DIGITS - 1)): the k1 entry starts the sum (Z = 1) and
    // the k2 entry is added to it as affine + affine (gejw_add_ge_z1).  That add meets no exceptional
    // case: its operands are +-(2a + 1) R and +-(2b + 1) lambda R with a, b < GLV_NT, equal or opposite
    // only if (2a + 1) == +-lambda (2b + 1) (mod n), R having order n, and no such pair exists
    // (tests/test_secp_recover_trim.py tries all of them).  u2 R = O cannot come out of it either.
    static_assert((GLV_DIGITS - 1) % DIG_PER_WORD == 0, "the top digit is the low slot of the last word");
    {
        ge9 P;
        uint32_t e1 = glv_slot<DIG_SLOT>(K1[DIG_WORDS - 1], GLV_DIGITS - 1) & (uint32_t)(GLV_NT - 1);
        uint32_t e2 = glv_slot<DIG_SLOT>(K2[DIG_WORDS - 1], GLV_DIGITS - 1) & (uint32_t)(GLV_NT - 1);
        GLV_ENTRY(P, e1, neg1, 0);
        acc.x = P.x;                     // 1 (an entry's x is a product's output)
        fe9_add(acc.y, P.y, P.y);        // W = 2y, 4
        fe9_normalize_weak(acc.y);       // 1
        GLV_ENTRY(P, e2, neg2, 1);
        gej9 t;
        gejw_add_ge_z1(t, acc, P);
        acc = t;
    }
    bool ainf = false;
#pragma unroll 1
    for (int i = GLV_DIGITS - 2; i >= 0; i--) {
#pragma unroll 1
        for (int d = 0; d < GLV_W; d++) gejw_dbl_neg(acc, acc);  // -2P each: + again after GLV_W
        // one add body, two passes: digit of k1 on T, digit of k2 on lambda(T) = (beta x, y)
#pragma unroll 1
        for (int j = 0; j < 2; j++) {
            uint32_t ei;
            bool dneg;
            glv_digit<GLV_W>(ei, dneg, glv_slot<DIG_SLOT>(j ? K2[DIG_WORDS - 2] : K1[DIG_WORDS - 2], i));
            ge9 P;
            GLV_ENTRY(P, ei, dneg != (j ? neg2 : neg1), j);
            gejw_add_ge(acc, ainf, acc, P);
        }
        if (i % DIG_PER_WORD == 0) {  // wave-uniform: the word is used up
            glv_next_word(K1);
            glv_next_word(K2);
        }
    }
#undef GLV_ENTRY
    gejw_to_gej9(acc, acc);  // (X, W, Z) -> Jacobian, Z magnitude 2
    fe9_mul(out.z, acc.z, zfac);  // back from E'' to the curve of (x, y) (2*1 -> 1)
    out.x = acc.x;
    out.y = acc.y;
    outinf = ainf;
#undef GLV_SET
#undef GLV_Y
#undef GLV_X
#undef GLV_L
}

}  // namespace gsv
