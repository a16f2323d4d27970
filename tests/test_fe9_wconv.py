"""Host build of the W-convention group operations of secp256k1_fe9.cuh — the GLV ladder's and the
comb's accumulators carry (X, W = 2Y, Z), the ladder's doubling returns -2P with six reductions
(gejw_dbl_neg) — and of the two fused products behind it, against affine Python arithmetic.

The extreme limb values of the fused products are in tests/test_asm_emulated_wconv.py (the
instruction emulator asserts every 64-bit chain); here the values, the alternating sign, the
exceptional cases of the mixed add, the conversion back and every output's limb bounds.  CPU-only."""
import ctypes
import random

import pytest

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
G = (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
     0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)
M29 = 2**29 - 1
U9, U18, U27 = ctypes.c_uint32 * 9, ctypes.c_uint32 * 18, ctypes.c_uint32 * 27


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    from conftest import build_native
    return build_native("fe9w_host.cpp", tmp_path_factory.mktemp("fe9w") / "fe9w_host.so")


# ---- affine reference (None = infinity)
def ec_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        l = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else:
        l = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (l * l - a[0] - b[0]) % P
    return (x, (l * (a[0] - x) - a[1]) % P)


def ec_mul(k, a):
    r = None
    while k:
        if k & 1:
            r = ec_add(r, a)
        a = ec_add(a, a)
        k >>= 1
    return r


def ec_neg(a):
    return (a[0], (P - a[1]) % P)


def val(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def from_int(x):
    return [(x >> (29 * i)) & M29 for i in range(9)]


def lift(l, rng):
    """the same value with limbs up to < 2^30: 2^29 borrowed from the limb above where it has one"""
    l = list(l)
    for i in range(8):
        if l[i + 1] > 0 and rng.random() < 0.7:
            l[i] += 1 << 29
            l[i + 1] -= 1
    return l


def wpoint(rng, pt, wmag2):
    """pt as (X, W, Z) limbs with a random Z; W canonical, or as the mixed add hands it over (a value's
    limbs doubled) / lifted to limbs < 2^30"""
    z = rng.randrange(1, P)
    X, Y = pt[0] * z * z % P, pt[1] * z**3 % P
    if wmag2 == 0:
        w = from_int(2 * Y % P)
    elif wmag2 == 1:
        w = [2 * x for x in from_int(Y)]
    else:
        w = lift(from_int(2 * Y % P), rng)
    return from_int(X) + w + from_int(z)


def w_affine(l):
    X, W, Z = val(l[0:9]) % P, val(l[9:18]) % P, val(l[18:27]) % P
    zi = pow(Z, -1, P)
    return (X * zi * zi % P, W * pow(2, -1, P) * zi**3 % P)


def j_affine(l):
    X, Y, Z = val(l[0:9]) % P, val(l[9:18]) % P, val(l[18:27]) % P
    zi = pow(Z, -1, P)
    return (X * zi * zi % P, Y * zi**3 % P)


def check_mag1(l):
    assert all(l[i] < 2**29 for i in (0, 1, 3, 4, 5, 6, 7)), l
    assert l[2] < 2**29 + 2**24 and l[8] < 2**24, l


def check_w2(l):
    """a product's output doubled limb-wise"""
    assert all(x % 2 == 0 for x in l)
    check_mag1([x // 2 for x in l])


def rnd_point(rng):
    return ec_mul(rng.randrange(1, N), G)


def test_fused_products(lib):
    rng = random.Random(71)
    r = U9()
    rl = lambda m: [rng.randrange(int(m * 2**29)) for _ in range(9)]
    for _ in range(300):
        a, b, c = rl(1.04), rl(6), rl(1.04)
        lib.w_dot_ms(r, U9(*a), U9(*b), U9(*c))
        check_mag1(list(r))
        assert val(r) % P == (val(a) * val(b) + val(c) ** 2) % P
        a = rl(1.33)
        lib.w_sqr3(r, U9(*a))
        check_mag1(list(r))
        assert val(r) % P == 3 * val(a) ** 2 % P


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_doublings_alternate_the_sign(lib, n):
    """n gejw_dbl_neg in a row: (-1)^n 2^n P, every coordinate at magnitude 1"""
    rng = random.Random(100 + n)
    r = U27()
    for it in range(40):
        pt = rnd_point(rng)
        lib.w_dbl_neg_n(r, U27(*wpoint(rng, pt, it % 3)), n)
        want = ec_mul(2**n, pt)
        assert w_affine(list(r)) == (want if n % 2 == 0 else ec_neg(want))
        for k in (0, 9, 18):
            check_mag1(list(r)[k:k + 9])


def test_plain_doubling(lib):
    """gejw_dbl (the mixed add's p == q case): +2P, W = Q_1 - a product's output (limbs < 2^30)"""
    rng = random.Random(5)
    r = U27()
    for it in range(40):
        pt = rnd_point(rng)
        lib.w_dbl(r, U27(*wpoint(rng, pt, it % 3)))
        assert w_affine(list(r)) == ec_mul(2, pt)
        check_mag1(list(r)[0:9])
        check_mag1(list(r)[18:27])
        assert all(x < 2**30 for x in list(r)[9:18])


def qlimbs(rng, q, mag2):
    x, y = from_int(q[0]), from_int(q[1])
    return (lift(x, rng) + lift(y, rng)) if mag2 else (x + y)


def test_mixed_add(lib):
    rng = random.Random(6)
    r = U27()
    for it in range(60):
        p, q = rnd_point(rng), rnd_point(rng)
        inf = lib.w_add_ge(r, U27(*wpoint(rng, p, it % 3)), 0, U18(*qlimbs(rng, q, it % 2)))
        assert inf == 0 and w_affine(list(r)) == ec_add(p, q)
        check_mag1(list(r)[0:9])
        check_w2(list(r)[9:18])
        check_mag1(list(r)[18:27])


def test_mixed_add_exceptional_cases(lib):
    rng = random.Random(7)
    r = U27()
    for it in range(12):
        p = rnd_point(rng)
        q = rnd_point(rng)
        # p == infinity (the accumulator's value is a placeholder): q, as (x, 2y, 1) at magnitude 1
        inf = lib.w_add_ge(r, U27(*wpoint(rng, p, it % 3)), 1, U18(*qlimbs(rng, q, it % 2)))
        assert inf == 0 and w_affine(list(r)) == q
        for k in (0, 9, 18):
            check_mag1(list(r)[k:k + 9])
        # p == q: the doubling, + 2P
        inf = lib.w_add_ge(r, U27(*wpoint(rng, p, it % 3)), 0, U18(*qlimbs(rng, p, it % 2)))
        assert inf == 0 and w_affine(list(r)) == ec_mul(2, p)
        check_mag1(list(r)[0:9])
        assert all(x < 2**30 for x in list(r)[9:18])
        check_mag1(list(r)[18:27])
        # p == -q: infinity
        inf = lib.w_add_ge(r, U27(*wpoint(rng, p, it % 3)), 0, U18(*qlimbs(rng, ec_neg(p), it % 2)))
        assert inf == 1


def test_conversion_back(lib):
    """(X, W, Z) -> the Jacobian (4X, 4W, 2Z): X, Y magnitude 1, Z magnitude 2"""
    rng = random.Random(8)
    r = U27()
    for it in range(40):
        pt = rnd_point(rng)
        lib.w_to_gej9(r, U27(*wpoint(rng, pt, it % 3)))
        assert j_affine(list(r)) == pt
        check_mag1(list(r)[0:9])
        check_mag1(list(r)[9:18])
        assert all(x < 2 * (2**29 + 2**24) for x in list(r)[18:27])


def test_ladder_step_and_why_the_window_is_even(lib):
    """four doublings and an add are 16 P + q; an ODD run before the add leaves the sum at
    -2^n P + q (GLV_W must be even: secp256k1_glv.cuh asserts it)"""
    rng = random.Random(9)
    r, s = U27(), U27()
    for it in range(10):
        p, q = rnd_point(rng), rnd_point(rng)
        ql = U18(*qlimbs(rng, q, it % 2))
        lib.w_dbl_neg_n(r, U27(*wpoint(rng, p, it % 3)), 4)
        assert lib.w_add_ge(s, r, 0, ql) == 0
        assert w_affine(list(s)) == ec_add(ec_mul(16, p), q)
        for n in (1, 3):
            lib.w_dbl_neg_n(r, U27(*wpoint(rng, p, it % 3)), n)
            assert lib.w_add_ge(s, r, 0, ql) == 0
            assert w_affine(list(s)) == ec_add(ec_neg(ec_mul(2**n, p)), q)
            assert w_affine(list(s)) != ec_add(ec_mul(2**n, p), q)
