// bigModExp (core/vm/contracts.go:226-252) for one item per lane on gfx950: b^e mod m over integers of
// caller-chosen length, in Montgomery arithmetic whose width is a template parameter.
//
// A number is L little-endian 32-bit limbs, limb i at x[i * S]: S = 1 for an array of the lane's own (the
// L = 8 class, where every index is a compile-time constant and the arrays are registers), S = 64 for a
// lane's column of a wave's lane-interleaved region of the work buffer or of LDS (the wider classes: a
// wave's load of limb i is one 256-byte line; modexp.hip says which number lives where).  FULL selects the register form: every limb loop is unrolled
// and runs over all L limbs; the memory form keeps the outer limb loops rolled and cuts the
// power-of-two half to the limbs it needs.
//
//   m = 0            zeros
//   m = 2^k q, q odd x1 = b^e mod q by Montgomery products (R = 2^(32 L); skipped for q = 1),
//                    x2 = b^e mod 2^k by truncated products, q^-1 mod 2^k by Newton lifting from the
//                    32-bit inverse, result = x1 + q ((x2 - x1) q^-1 mod 2^k); k = 0 is x1 alone
//   setup            R mod q by doublings from 2^(bitlen(q) - 1), 32 more doublings and log2(L) Montgomery
//                    squarings give R^2 mod q (mont(2^s R, 2^t R) = 2^(s+t) R); the base enters as
//                    mont(piece, R^2), by Horner over L-limb pieces when it is longer than L limbs
//   exponent         plain binary from the lane's top set bit (the exponent is public: variable time);
//                    the square is the general product with both operands the same.  Measured and not
//                    kept: a 4-bit fixed window with the 15-entry table in LDS (32 KiB a wave) ran the
//                    32/32/32 shape in 8.55 ms against 6.82 ms (profiles/modexp/sweep.json)
// Free of HIP when compiled by a host compiler (tests/native/modexp_host_main.cpp runs it under ASan).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MDX_FN __device__ __forceinline__
#define MDX_PRAGMA(x) _Pragma(#x)
#define MDX_UNROLL(n) MDX_PRAGMA(unroll n)
#else
#define MDX_FN static inline
#define MDX_UNROLL(n)
#endif

namespace gsv {
namespace mdx {

typedef unsigned long long u64;

// the six numbers a lane works on (L limbs each, stride S); t is the products' accumulator and a temporary
struct Slots {
    uint32_t *q, *t, *xr, *acc, *r2, *aux;
};

// -q^-1 mod 2^32 for odd q
MDX_FN uint32_t neg_inv32(uint32_t q0) {
    uint32_t x = q0;  // q0 * q0 = 1 mod 8
    for (int i = 0; i < 4; i++) x *= 2u - q0 * x;
    return 0u - x;
}

// limbs [0, cnt) of (the big-endian number b[0 .. len)) >> bitoff; limbs from cnt up are not written
template <int L, int S, int U>
MDX_FN void load_bits(uint32_t* x, const uint8_t* b, uint32_t len, uint32_t bitoff, int cnt) {
    MDX_UNROLL(U)
    for (int i = 0; i < L; i++) {
        if (i < cnt) {
            const uint32_t bit = bitoff + 32u * (uint32_t)i, p = bit >> 3, sh = bit & 7;
            u64 v = 0;
            for (uint32_t k = 0; k < 5; k++)
                if (p + k < len) v |= (u64)b[len - 1 - (p + k)] << (8 * k);
            x[i * S] = (uint32_t)(v >> sh);
        }
    }
}

// the low mod_len bytes of x, big-endian
template <int L, int S, int U>
MDX_FN void store_be(uint8_t* out, uint32_t len, const uint32_t* x) {
    MDX_UNROLL(U)
    for (int i = 0; i < L; i++) {
        if (4u * (uint32_t)i < len) {
            const uint32_t v = x[i * S];
            for (uint32_t k = 0; k < 4; k++) {
                const uint32_t pos = 4u * (uint32_t)i + k;
                if (pos < len) out[len - 1 - pos] = (uint8_t)(v >> (8 * k));
            }
        }
    }
}

MDX_FN void store_zero(uint8_t* out, uint32_t len) {
    for (uint32_t i = 0; i < len; i++) out[i] = 0;
}

template <int L, int S, int U>
MDX_FN void set_small(uint32_t* x, uint32_t v) {
    MDX_UNROLL(U)
    for (int i = 0; i < L; i++) x[i * S] = i == 0 ? v : 0u;
}

template <int L, int S, int U>
MDX_FN void copy(uint32_t* d, const uint32_t* s, int cnt) {
    MDX_UNROLL(U)
    for (int i = 0; i < L; i++)
        if (i < cnt) d[i * S] = s[i * S];
}

// x >= q
template <int L, int S, int U>
MDX_FN bool geq(const uint32_t* x, const uint32_t* q) {
    bool ge = true;
    MDX_UNROLL(U)
    for (int i = 0; i < L; i++) {  // the highest limb that differs decides: it is looked at last
        const uint32_t a = x[i * S], b = q[i * S];
        if (a != b) ge = a > b;
    }
    return ge;
}

// d = x - (take ? q : 0)
template <int L, int S, int U>
MDX_FN void sub_if(uint32_t* d, const uint32_t* x, const uint32_t* q, bool take) {
    uint32_t bw = 0;
    MDX_UNROLL(U)
    for (int i = 0; i < L; i++) {
        const u64 v = (u64)x[i * S] - (take ? q[i * S] : 0u) - bw;
        d[i * S] = (uint32_t)v;
        bw = (uint32_t)(v >> 32) & 1u;
    }
}

// x = 2 x mod q for x < q
template <int L, int S, int U>
MDX_FN void dbl_mod(uint32_t* x, const uint32_t* q) {
    uint32_t c = 0;
    MDX_UNROLL(U)
    for (int i = 0; i < L; i++) {
        const uint32_t v = x[i * S];
        x[i * S] = (v << 1) | c;
        c = v >> 31;
    }
    sub_if<L, S, U>(x, x, q, c || geq<L, S, U>(x, q));
}

// x = x + y mod q for x, y < q
template <int L, int S, int U>
MDX_FN void add_mod(uint32_t* x, const uint32_t* y, const uint32_t* q) {
    uint32_t c = 0;
    MDX_UNROLL(U)
    for (int i = 0; i < L; i++) {
        const u64 v = (u64)x[i * S] + y[i * S] + c;
        x[i * S] = (uint32_t)v;
        c = (uint32_t)(v >> 32);
    }
    sub_if<L, S, U>(x, x, q, c || geq<L, S, U>(x, q));
}

// The Montgomery product's limb loops (finely integrated operand scanning: one pass over t per limb of
// a, two carry chains): t + top 2^(32 L) = a b / R mod q, below b + q.  t is no operand.
template <int L, int S, int U, int UJ>
MDX_FN uint32_t mont_core(uint32_t* __restrict__ t, const uint32_t* a, const uint32_t* b, const uint32_t* q,
                          uint32_t n0) {
    MDX_UNROLL(U)
    for (int i = 0; i < L; i++) t[i * S] = 0;
    uint32_t top = 0;
    MDX_UNROLL(U)
    for (int i = 0; i < L; i++) {
        const uint32_t ai = a[i * S];
        u64 s = (u64)t[0] + (u64)ai * b[0];
        const uint32_t u = (uint32_t)s * n0;
        u64 r = (u64)(uint32_t)s + (u64)u * q[0];
        uint32_t c1 = (uint32_t)(s >> 32), c2 = (uint32_t)(r >> 32);
        MDX_UNROLL(UJ)
        for (int j = 1; j < L; j++) {
            s = (u64)ai * b[j * S] + t[j * S] + c1;
            c1 = (uint32_t)(s >> 32);
            r = (u64)u * q[j * S] + (uint32_t)s + c2;
            c2 = (uint32_t)(r >> 32);
            t[(j - 1) * S] = (uint32_t)r;
        }
        s = (u64)top + c1 + c2;
        t[(L - 1) * S] = (uint32_t)s;
        top = (uint32_t)(s >> 32);
    }
    return top;
}

// d = a b / R mod q for b < q (a < R); d may be a or b
template <int L, int S, int U, int UJ>
MDX_FN void mont(uint32_t* d, const uint32_t* a, const uint32_t* b, const uint32_t* q, uint32_t n0, uint32_t* t) {
    const uint32_t top = mont_core<L, S, U, UJ>(t, a, b, q, n0);
    sub_if<L, S, U>(d, t, q, top || geq<L, S, U>(t, q));
}

// d = the low n limbs of a b, a of na limbs (na <= n); d is no operand.  The register form takes
// na = n = L.
template <int L, int S, int U, bool FULL>
MDX_FN void mul_lo(uint32_t* __restrict__ d, const uint32_t* a, int na, const uint32_t* b, int n) {
    const int NA = FULL ? L : na, N = FULL ? L : n;
    MDX_UNROLL(U)
    for (int i = 0; i < L; i++)
        if (i < N) d[i * S] = 0;
    MDX_UNROLL(U)
    for (int i = 0; i < L; i++) {
        if (i < NA) {
            const uint32_t ai = a[i * S];
            uint32_t c = 0;
            MDX_UNROLL(U)
            for (int j = 0; j < N - i; j++) {  // the carry out of limb n - 1 is cut off
                const u64 s = (u64)ai * b[j * S] + d[(i + j) * S] + c;
                d[(i + j) * S] = (uint32_t)s;
                c = (uint32_t)(s >> 32);
            }
        }
    }
}

// the exponent's bit length (0 for e = 0): leading zero bytes are skipped once
MDX_FN uint32_t exp_bits(const uint8_t* e, uint32_t el) {
    uint32_t i = 0;
    while (i < el && e[i] == 0) i++;
    if (i == el) return 0;
    return 8 * (el - 1 - i) + (32 - (uint32_t)__builtin_clz((uint32_t)e[i]));
}
MDX_FN uint32_t exp_bit(const uint8_t* e, uint32_t el, uint32_t bit) { return (e[el - 1 - (bit >> 3)] >> (bit & 7)) & 1u; }

// One item: in = base || exp || mod (bl, el, ml bytes, big-endian, any alignment), out = ml bytes.
// ml <= 4 L; the six numbers of w are the lane's own.
template <int L, int S, bool FULL>
MDX_FN void modexp_item(const uint8_t* in, uint32_t bl, uint32_t el, uint32_t ml, uint8_t* out, const Slots& w) {
    constexpr int U = FULL ? L : 1, UJ = FULL ? L : 4;
    const uint8_t *bb = in, *eb = in + bl, *mb = in + bl + el;
    uint32_t *q = w.q, *t = w.t, *xr = w.xr, *acc = w.acc, *r2 = w.r2, *aux = w.aux;

    // m, its trailing zero bits k and its bit length
    load_bits<L, S, U>(q, mb, ml, 0, L);
    uint32_t k = 0, mbits = 0;
    {
        bool seen = false;
        MDX_UNROLL(U)
        for (int i = 0; i < L; i++) {
            const uint32_t v = q[i * S];
            if (v) {
                if (!seen) k = 32u * (uint32_t)i + (uint32_t)__builtin_ctz(v);
                seen = true;
                mbits = 32u * (uint32_t)i + 32u - (uint32_t)__builtin_clz(v);
            }
        }
        if (!seen) {
            store_zero(out, ml);
            return;
        }
    }
    if (k) load_bits<L, S, U>(q, mb, ml, k, L);  // q = m >> k, odd
    const uint32_t qbits = mbits - k;
    const uint32_t ebits = exp_bits(eb, el);

    // x1 = b^e mod q -> acc
    if (qbits == 1) {
        set_small<L, S, U>(acc, 0);
    } else if (ebits == 0) {
        set_small<L, S, U>(acc, 1);
    } else {
        const uint32_t n0 = neg_inv32(q[0]);
        // r2 = R^2 mod q
        MDX_UNROLL(U)
        for (int i = 0; i < L; i++)
            r2[i * S] = (uint32_t)i == (qbits - 1) / 32 ? 1u << ((qbits - 1) & 31) : 0u;
        for (uint32_t i = qbits - 1; i < 32u * L + 32u; i++) dbl_mod<L, S, U>(r2, q);  // 2^32 R mod q
        for (int s = 1; s < L; s *= 2) mont<L, S, U, UJ>(r2, r2, r2, q, n0, t);
        // xr = b R mod q
        const uint32_t pieces = bl ? (bl + 4u * L - 1) / (4u * L) : 1;
        load_bits<L, S, U>(aux, bb, bl, (pieces - 1) * 32u * L, L);
        mont<L, S, U, UJ>(xr, aux, r2, q, n0, t);
        for (uint32_t p = pieces - 1; p-- > 0;) {
            mont<L, S, U, UJ>(xr, xr, r2, q, n0, t);
            load_bits<L, S, U>(aux, bb, bl, p * 32u * L, L);
            mont<L, S, U, UJ>(aux, aux, r2, q, n0, t);
            add_mod<L, S, U>(xr, aux, q);
        }
        // the walk
        copy<L, S, U>(acc, xr, L);
        for (uint32_t bit = ebits - 1; bit-- > 0;) {
            mont<L, S, U, UJ>(acc, acc, acc, q, n0, t);
            if (exp_bit(eb, el, bit)) mont<L, S, U, UJ>(acc, acc, xr, q, n0, t);
        }
        set_small<L, S, U>(r2, 1);
        mont<L, S, U, UJ>(acc, acc, r2, q, n0, t);
    }
    if (k == 0) {
        store_be<L, S, U>(out, ml, acc);
        return;
    }

    // x2 = b^e mod 2^(32 K) -> r2
    const int K = FULL ? L : (int)((k + 31) / 32);
    if (ebits == 0) {
        set_small<L, S, U>(r2, 1);
    } else {
        load_bits<L, S, U>(xr, bb, bl, 0, K);
        copy<L, S, U>(r2, xr, K);
        for (uint32_t bit = ebits - 1; bit-- > 0;) {
            mul_lo<L, S, U, FULL>(t, r2, K, r2, K);
            copy<L, S, U>(r2, t, K);
            if (exp_bit(eb, el, bit)) {
                mul_lo<L, S, U, FULL>(t, r2, K, xr, K);
                copy<L, S, U>(r2, t, K);
            }
        }
    }
    // aux = q^-1 mod 2^(32 K): each step doubles the bits that are right
    set_small<L, S, U>(aux, 0u - neg_inv32(q[0]));
    for (int bits = 32; bits < 32 * K; bits *= 2) {
        mul_lo<L, S, U, FULL>(t, aux, K, q, K);
        uint32_t bw = 0;
        MDX_UNROLL(U)
        for (int i = 0; i < L; i++) {  // t = 2 - t
            if (i < K) {
                const u64 v = (u64)(i == 0 ? 2u : 0u) - t[i * S] - bw;
                t[i * S] = (uint32_t)v;
                bw = (uint32_t)(v >> 32) & 1u;
            }
        }
        mul_lo<L, S, U, FULL>(xr, aux, K, t, K);
        copy<L, S, U>(aux, xr, K);
    }
    // h = (x2 - x1) q^-1 mod 2^k -> t
    {
        uint32_t bw = 0;
        MDX_UNROLL(U)
        for (int i = 0; i < L; i++) {
            if (i < K) {
                const u64 v = (u64)r2[i * S] - acc[i * S] - bw;
                r2[i * S] = (uint32_t)v;
                bw = (uint32_t)(v >> 32) & 1u;
            }
        }
    }
    mul_lo<L, S, U, FULL>(t, r2, K, aux, K);
    MDX_UNROLL(U)
    for (int i = 0; i < L; i++) {
        if (i < K) {
            const uint32_t lo = 32u * (uint32_t)i;
            if (lo >= k) t[i * S] = 0;
            else if (k - lo < 32) t[i * S] &= (1u << (k - lo)) - 1u;
        }
    }
    // result = x1 + q h (below m, so L limbs hold it) -> xr
    mul_lo<L, S, U, FULL>(xr, t, K, q, L);
    {
        uint32_t c = 0;
        MDX_UNROLL(U)
        for (int i = 0; i < L; i++) {
            const u64 v = (u64)xr[i * S] + acc[i * S] + c;
            xr[i * S] = (uint32_t)v;
            c = (uint32_t)(v >> 32);
        }
    }
    store_be<L, S, U>(out, ml, xr);
}

}  // namespace mdx
}  // namespace gsv
