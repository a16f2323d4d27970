// Host build of secp256k1_fe9.cuh's products with subtrahends (fe9_mul_sub, fe9_sqr_sub2, fe9_sqr_sub_2x:
// the C++ the device runs under FE9_NO_ASM) and of the group formulas rewired onto them, beside the
// compositions they replace (fe9_neg / fe9_negsum into fe9_mul_add / fe9_sqr_add, restated below as
// ref_*), exported for tests/test_fe9_signed.py.
#include "../../geth-sharding_amd/csrc/secp256k1_fe9.cuh"
using namespace gsv;
static void ldf(fe9& x, const uint32_t* a) { for (int i = 0; i < 9; i++) x.v[i] = a[i]; }
static void stf(uint32_t* r, const fe9& x) { for (int i = 0; i < 9; i++) r[i] = x.v[i]; }
static void ld(gej9& a, const uint32_t* p) { ldf(a.x, p); ldf(a.y, p + 9); ldf(a.z, p + 18); }
static void st(uint32_t* r, const gej9& o) { stf(r, o.x); stf(r + 9, o.y); stf(r + 18, o.z); }
static void ldg(ge9& a, const uint32_t* p) { ldf(a.x, p); ldf(a.y, p + 9); }
static void stg(uint32_t* r, const ge9& o) { stf(r, o.x); stf(r + 9, o.y); }

// ---- the replaced compositions
static void ref_dbl_neg(gej9& r, const gej9& p) {
    fe9 B, D, E, t, u;
    fe9_sqr3(E, p.x);
    fe9_sqr(B, p.y);
    fe9_mul(D, p.x, B);
    fe9_mul(r.z, p.y, p.z);
    fe9_negsum<2>(t, D, D);
    fe9_sqr_add(u, E, t);
    fe9_sub<1>(t, u, D);
    fe9_add(t, t, t);
    fe9_dot_ms(r.y, E, t, B);
    r.x = u;
}
static void ref_add_ge_core(gej9& o, fe9& h, fe9& rr, const gej9& p, const ge9& q) {
    fe9 z1z1, s2, hh, i4, j, v, t, w;
    fe9_sqr(z1z1, p.z);
    fe9_neg<1>(t, p.x);
    fe9_mul_add(h, q.x, z1z1, t);
    fe9_mul(s2, q.y, p.z);
    fe9_add(s2, s2, s2);
    fe9_neg<2>(t, p.y);
    fe9_mul_add(rr, s2, z1z1, t);
    fe9_sqr(hh, h);
    fe9_mul_small(i4, hh, 4);
    fe9_mul(j, h, i4);
    fe9_mul(v, p.x, i4);
    fe9_negsum3<3>(t, j, v, v);
    fe9_sqr_add(o.x, rr, t);
    fe9_sub<1>(t, v, o.x);
    fe9_neg<1>(w, j);
    fe9_dot(o.y, rr, t, p.y, w);
    fe9_add(o.y, o.y, o.y);
    fe9_add(t, p.z, h);
    fe9_negsum<2>(w, z1z1, hh);
    fe9_sqr_add(o.z, t, w);
}
static void ref_add_ge_z1(gej9& o, const gej9& p, const ge9& q) {
    fe9 h, rr, hh, i4, j, v, t, w;
    fe9_sub<1>(h, q.x, p.x);
    fe9_normalize_weak(h);
    fe9_add(t, q.y, q.y);
    fe9_sub<2>(rr, t, p.y);
    fe9_normalize_weak(rr);
    fe9_sqr(hh, h);
    fe9_mul_small(i4, hh, 4);
    fe9_mul(j, h, i4);
    fe9_mul(v, p.x, i4);
    fe9_negsum3<3>(t, j, v, v);
    fe9_sqr_add(o.x, rr, t);
    fe9_sub<1>(t, v, o.x);
    fe9_neg<1>(w, j);
    fe9_dot(o.y, rr, t, p.y, w);
    fe9_add(o.y, o.y, o.y);
    fe9_add(o.z, h, h);
    fe9_normalize_weak(o.z);
}
static void ref_dblu(ge9& d, ge9& rp, fe9& z, const fe9& x, const fe9& y) {
    fe9 A, B, t, C4, E, u;
    fe9_sqr(A, x);
    fe9_sqr(B, y);
    fe9_mul_small(t, B, 4);
    fe9_mul(rp.x, x, t);
    fe9_add(t, B, B);
    fe9_sqr(C4, t);
    fe9_mul_small(E, A, 3);
    fe9_normalize_weak(E);
    fe9_add(z, y, y);
    fe9_negsum<2>(t, rp.x, rp.x);
    fe9_sqr_add(d.x, E, t);
    fe9_sub<1>(u, rp.x, d.x);
    fe9_negsum<2>(t, C4, C4);
    fe9_mul_add(d.y, E, u, t);
    fe9_add(rp.y, C4, C4);
    fe9_normalize_weak(rp.y);
}
static void ref_zaddu(ge9& s, ge9& p1, fe9& zr, const ge9& p2) {
    fe9 C, W1, W2, rr, t, u, A1;
    fe9_sub<1>(zr, p1.x, p2.x);
    fe9_normalize_weak(zr);
    fe9_sqr(C, zr);
    fe9_mul(W1, p1.x, C);
    fe9_mul(W2, p2.x, C);
    fe9_sub<1>(rr, p1.y, p2.y);
    fe9_normalize_weak(rr);
    fe9_negsum<2>(t, W1, W2);
    fe9_sqr_add(s.x, rr, t);
    fe9_sub<1>(t, W1, W2);
    fe9_mul(A1, p1.y, t);
    fe9_sub<1>(u, W1, s.x);
    fe9_neg<1>(t, A1);
    fe9_mul_add(s.y, rr, u, t);
    p1.x = W1;
    p1.y = A1;
}

extern "C" {
// which: 0 the new statement, 1 the replaced composition.  cm: the subtrahend's magnitude bound (1..3)
void s_mul_sub(uint32_t* r, const uint32_t* a, const uint32_t* b, const uint32_t* c, int cm, int which) {
    fe9 x, y, z, t, o; ldf(x, a); ldf(y, b); ldf(z, c);
    if (!which) fe9_mul_sub(o, x, y, z);
    else {
        if (cm == 1) fe9_neg<1>(t, z); else if (cm == 2) fe9_neg<2>(t, z); else fe9_neg<3>(t, z);
        fe9_mul_add(o, x, y, t);
    }
    stf(r, o);
}
// a^2 - c - kd d (c, d at magnitude 1); kd = 0: a^2 - 2 d
void s_sqr_sub2(uint32_t* r, const uint32_t* a, const uint32_t* c, const uint32_t* d, int kd, int which) {
    fe9 x, y, z, t, o; ldf(x, a); ldf(y, c); ldf(z, d);
    if (!which) {
        if (kd == 0) fe9_sqr_sub_2x(o, x, z); else if (kd == 1) fe9_sqr_sub2<1>(o, x, y, z); else fe9_sqr_sub2<2>(o, x, y, z);
    } else {
        if (kd == 0) fe9_negsum<2>(t, z, z); else if (kd == 1) fe9_negsum<2>(t, y, z); else fe9_negsum3<3>(t, y, z, z);
        fe9_sqr_add(o, x, t);
    }
    stf(r, o);
}
void s_dbl_neg(uint32_t* r, const uint32_t* p, int which) {
    gej9 a, o; ld(a, p);
    if (which) ref_dbl_neg(o, a); else gejw_dbl_neg(o, a);
    st(r, o);
}
// r: (X, W, Z), then H and rr (45 words)
void s_add_ge_core(uint32_t* r, const uint32_t* p, const uint32_t* q, int which) {
    gej9 a, o; ge9 b; fe9 h, rr; ld(a, p); ldg(b, q);
    if (which) ref_add_ge_core(o, h, rr, a, b); else gejw_add_ge_core(o, h, rr, a, b);
    st(r, o); stf(r + 27, h); stf(r + 36, rr);
}
int s_add_ge(uint32_t* r, const uint32_t* p, int pinf, const uint32_t* q) {
    gej9 a, o; ge9 b; ld(a, p); ldg(b, q);
    bool inf = pinf != 0; gejw_add_ge(o, inf, a, b); st(r, o); return inf;
}
void s_add_ge_z1(uint32_t* r, const uint32_t* p, const uint32_t* q, int which) {
    gej9 a, o; ge9 b; ld(a, p); ldg(b, q);
    if (which) ref_add_ge_z1(o, a, b); else gejw_add_ge_z1(o, a, b);
    st(r, o);
}
// r: d (18), rp (18), z (9)
void s_dblu(uint32_t* r, const uint32_t* x, const uint32_t* y, int which) {
    ge9 d, rp; fe9 z, fx, fy; ldf(fx, x); ldf(fy, y);
    if (which) ref_dblu(d, rp, z, fx, fy); else ge9_dblu(d, rp, z, fx, fy);
    stg(r, d); stg(r + 18, rp); stf(r + 36, z);
}
// r: s (18), p1 rescaled (18), zr (9)
void s_zaddu(uint32_t* r, const uint32_t* p1, const uint32_t* p2, int which) {
    ge9 s, a, b; fe9 zr; ldg(a, p1); ldg(b, p2);
    if (which) ref_zaddu(s, a, zr, b); else ge9_zaddu(s, a, zr, b);
    stg(r, s); stg(r + 18, a); stf(r + 36, zr);
}
}
