// Host build of secp256k1_fe9.cuh's fused products and W-convention group operations
// ((X, W = 2Y, Z): gejw_dbl_neg, gejw_add_ge, gejw_to_gej9), exported for tests/test_fe9_wconv.py.
#include "../../geth-sharding_amd/csrc/secp256k1_fe9.cuh"
using namespace gsv;
static void ldf(fe9& x, const uint32_t* a) { for (int i = 0; i < 9; i++) x.v[i] = a[i]; }
static void stf(uint32_t* r, const fe9& x) { for (int i = 0; i < 9; i++) r[i] = x.v[i]; }
static void ld(gej9& a, const uint32_t* p) { ldf(a.x, p); ldf(a.y, p + 9); ldf(a.z, p + 18); }
static void st(uint32_t* r, const gej9& o) { stf(r, o.x); stf(r + 9, o.y); stf(r + 18, o.z); }
extern "C" {
void w_dot_ms(uint32_t* r, const uint32_t* a, const uint32_t* b, const uint32_t* c) {
    fe9 x, y, z, o; ldf(x, a); ldf(y, b); ldf(z, c); fe9_dot_ms(o, x, y, z); stf(r, o);
}
void w_sqr3(uint32_t* r, const uint32_t* a) { fe9 x, o; ldf(x, a); fe9_sqr3(o, x); stf(r, o); }
// p, r = 27 words (X, W, Z); n doublings in place, as the ladder runs them
void w_dbl_neg_n(uint32_t* r, const uint32_t* p, int n) {
    gej9 a; ld(a, p);
    for (int i = 0; i < n; i++) gejw_dbl_neg(a, a);
    st(r, a);
}
void w_dbl(uint32_t* r, const uint32_t* p) { gej9 a, o; ld(a, p); gejw_dbl(o, a); st(r, o); }
int w_add_ge(uint32_t* r, const uint32_t* p, int pinf, const uint32_t* q) {
    gej9 a, o; ge9 b; ld(a, p); ldf(b.x, q); ldf(b.y, q + 9);
    bool inf = pinf != 0; gejw_add_ge(o, inf, a, b); st(r, o); return inf;
}
void w_to_gej9(uint32_t* r, const uint32_t* p) { gej9 a, o; ld(a, p); gejw_to_gej9(o, a); st(r, o); }
}
