// Host build of what the secp256k1 recovery reads outside its two ladder bodies, exported for
// tests/test_secp_recover_trim.py: the ladder's digits taken from the scalar's bits and the split's
// short products (glv_sched.cuh), the affine + affine add of a sum's first step and the one-limb
// filter in front of the exceptional-case test (secp256k1_fe9.cuh).  TRIM_W / TRIM_DIGITS are the
// device's GLV_W / GLV_DIGITS, passed by the test from tests/secp_glv_model.py.
#include "../../geth-sharding_amd/csrc/secp256k1_fe9.cuh"
#include "../../geth-sharding_amd/csrc/glv_sched.cuh"
using namespace gsv;
static_assert(TRIM_W == 4 && TRIM_DIGITS == 33, "the word count below is for 33 4-bit slots");
constexpr int NW = 5;
static void ldf(fe9& x, const uint32_t* a) { for (int i = 0; i < 9; i++) x.v[i] = a[i]; }
static void stf(uint32_t* r, const fe9& x) { for (int i = 0; i < 9; i++) r[i] = x.v[i]; }
extern "C" {
// codes[TRIM_DIGITS] of the odd magnitude k (8 words): sign bit above the table index for the digits
// below the top, the top digit's slot as it is; n scalars in a row
void t_digit_codes(uint8_t* codes, const uint32_t* k, int n) {
    for (int s = 0; s < n; s++, k += 8, codes += TRIM_DIGITS) {
        uint32_t K[NW];
        glv_halve(K, k);
        // the ladder's walk: the top digit from the last word, then the words from the top down
        codes[TRIM_DIGITS - 1] = (uint8_t)glv_slot<TRIM_W>(K[NW - 1], TRIM_DIGITS - 1);
        for (int i = TRIM_DIGITS - 2; i >= 0; i--) {
            uint32_t idx;
            bool neg;
            glv_digit<TRIM_W>(idx, neg, glv_slot<TRIM_W>(K[NW - 2], i));
            codes[i] = (uint8_t)(((neg ? 1u : 0u) << (TRIM_W - 1)) | idx);
            if (i % (32 / TRIM_W) == 0) glv_next_word(K);
        }
    }
}
void t_short_r2(uint32_t* r2, const uint32_t* c1, const uint32_t* nb1, const uint32_t* c2, const uint32_t* b2,
                const uint32_t* n) {
    glv_short_r2(r2, c1, nb1, c2, b2, n);
}
// p = 27 words (X, W, Z: Z is not read), q = 18 words (x, y); r = 27 words (X, W, Z)
void t_add_z1(uint32_t* r, const uint32_t* p, const uint32_t* q) {
    gej9 a, o;
    ge9 b;
    ldf(a.x, p); ldf(a.y, p + 9); ldf(a.z, p + 18);
    ldf(b.x, q); ldf(b.y, q + 9);
    gejw_add_ge_z1(o, a, b);
    stf(r, o.x); stf(r + 9, o.y); stf(r + 18, o.z);
}
// the add whose caller rules the exceptional cases out: the identity start is all it handles
int t_add_nx(uint32_t* r, const uint32_t* p, int pinf, const uint32_t* q) {
    gej9 a, o;
    ge9 b;
    ldf(a.x, p); ldf(a.y, p + 9); ldf(a.z, p + 18);
    ldf(b.x, q); ldf(b.y, q + 9);
    bool inf = pinf != 0;
    gejw_add_ge_nx(o, inf, a, b);
    stf(r, o.x); stf(r + 9, o.y); stf(r + 18, o.z);
    return inf;
}
int t_filter(const uint32_t* a) { fe9 x; ldf(x, a); return fe9_maybe_zero_weak(x) ? 1 : 0; }
int t_zero_weak(const uint32_t* a) { fe9 x; ldf(x, a); return fe9_is_zero_weak(x) ? 1 : 0; }
// n weak values whose limbs are drawn 0 / p's limb / random in the weak form's range (so that zero
// and p come up): out = {values that are zero, values the filter passes, zero values the filter missed}
void t_filter_sweep(uint64_t* out, uint64_t seed, uint32_t n, uint32_t pct_special) {
    uint64_t s = seed | 1;
    auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    out[0] = out[1] = out[2] = 0;
    for (uint32_t it = 0; it < n; it++) {
        fe9 x;
        for (int i = 0; i < 9; i++) {
            uint64_t r = next();
            uint32_t bound = i == 8 ? (1u << 24) : i == 2 ? (1u << 29) + (1u << 24) : (1u << 29);
            uint32_t pick = (uint32_t)(r >> 40) % 100u;
            x.v[i] = pick < pct_special / 2 ? 0u : pick < pct_special ? FE9_P[i] : (uint32_t)(r % bound);
        }
        bool z = fe9_is_zero_weak(x), f = fe9_maybe_zero_weak(x);
        out[0] += z;
        out[1] += f;
        out[2] += z && !f;
    }
}
}
