"""Host build of the products with subtrahends of secp256k1_fe9.cuh (fe9_mul_sub, fe9_sqr_sub2,
fe9_sqr_sub_2x: the C++ that restates the generated statements, what the device runs under FE9_NO_ASM)
and of the group formulas rewired onto them (gejw_dbl_neg, gejw_add_ge_core, gejw_add_ge_z1, ge9_dblu,
ge9_zaddu), against the compositions they replace (fe9_neg / fe9_negsum into fe9_mul_add / fe9_sqr_add;
tests/native/fe9s_host.cpp restates them) and against Python integers.

"Equal" is equality of the field element: both forms add a multiple of p to stay non-negative (Q_M there,
8192 p here), a different one, so the weakly normalised limbs may differ by p.  Every output's limb bounds
are checked as well.  The instruction-level bounds are in tests/test_asm_emulated_signed.py.  CPU-only."""
import ctypes
import random

import pytest

from test_fe9_wconv import (G, N, P, U9, U18, U27, check_mag1, check_w2, ec_add, ec_mul, ec_neg, from_int, lift,
                            qlimbs, rnd_point, val, w_affine, wpoint)

U45 = ctypes.c_uint32 * 45
SUB_MAX = [2**31 - 1] * 9


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    from conftest import build_native
    return build_native("fe9s_host.cpp", tmp_path_factory.mktemp("fe9s") / "fe9s_host.so")


def limbs_at(m):
    return [int(m * 2**29) - 1] * 9


def rl(rng, m):
    return [rng.randrange(int(m * 2**29)) for _ in range(9)]


def prod_max():
    l = [2**29 - 1] * 9
    l[2] = 2**29 + 2**24 - 1
    l[8] = 2**24 - 1
    return l


def both(fn, *args):
    r, o = U9(), U9()
    fn(r, *args, 0)
    fn(o, *args, 1)
    return list(r), list(o)


# ---------------------------------------------------------------- the statements
MUL_MAGS = [(1.04, 3.36), (3.36, 1.04), (2, 1.75), (1.87, 1.87)]


def test_mul_sub_equals_the_composition(lib):
    rng = random.Random(31)
    cases = [(limbs_at(ma), limbs_at(mb), limbs_at(cm), cm) for (ma, mb) in MUL_MAGS for cm in (1, 2, 3)]
    cases += [(limbs_at(ma), limbs_at(mb), [0] * 9, 1) for (ma, mb) in MUL_MAGS]
    cases += [([0] * 9, [0] * 9, limbs_at(cm), cm) for cm in (1, 2, 3)]
    for it in range(10000):
        ma, mb = MUL_MAGS[it % 4]
        cm = 1 + it % 3
        cases.append((rl(rng, ma), rl(rng, mb), rl(rng, cm), cm))
    for a, b, c, cm in cases:
        new, old = both(lib.s_mul_sub, U9(*a), U9(*b), U9(*c), cm)
        want = (val(a) * val(b) - val(c)) % P
        assert val(new) % P == want and val(old) % P == want
        check_mag1(new)


def test_mul_sub_at_the_largest_subtrahend(lib):
    """limbs of 2^31 - 1 (above what fe9_neg admits: Python integers only), products at their maxima and at 0"""
    r = U9()
    for a, b in [(limbs_at(ma), limbs_at(mb)) for (ma, mb) in MUL_MAGS] + [([0] * 9, [0] * 9)]:
        lib.s_mul_sub(r, U9(*a), U9(*b), U9(*SUB_MAX), 3, 0)
        assert val(r) % P == (val(a) * val(b) - val(SUB_MAX)) % P
        check_mag1(list(r))


@pytest.mark.parametrize("kd", [0, 1, 2])
def test_sqr_sub2_equals_the_composition(lib, kd):
    """kd = 0: a^2 - 2d; 1: a^2 - c - d; 2: a^2 - c - 2d, with c, d at magnitude 1 (what negsum<2> / negsum3<3>
    admit), a up to 1.87"""
    rng = random.Random(32 + kd)
    mags = (1.04, 1.5, 1.87)
    cases = [(limbs_at(m), s, s) for m in mags for s in (limbs_at(1), prod_max(), [0] * 9)]
    cases += [([0] * 9, limbs_at(1), limbs_at(1))]
    for it in range(10000):
        cases.append((rl(rng, mags[it % 3]), rl(rng, 1), rl(rng, 1)))
    for a, c, d in cases:
        new, old = both(lib.s_sqr_sub2, U9(*a), U9(*c), U9(*d), kd)
        want = (val(a) ** 2 - (val(c) if kd else 0) - (kd or 2) * val(d)) % P
        assert val(new) % P == want and val(old) % P == want
        check_mag1(new)
    r = U9()
    for a in (limbs_at(1.87), [0] * 9):  # subtrahends of 2^31 - 1: Python integers only
        lib.s_sqr_sub2(r, U9(*a), U9(*SUB_MAX), U9(*SUB_MAX), kd, 0)
        assert val(r) % P == (val(a) ** 2 - (val(SUB_MAX) if kd else 0) - (kd or 2) * val(SUB_MAX)) % P
        check_mag1(list(r))


# ---------------------------------------------------------------- the rewired formulas
def same_field_elements(new, old, n):
    assert len(new) == len(old) == 9 * n
    for k in range(0, 9 * n, 9):
        assert val(new[k:k + 9]) % P == val(old[k:k + 9]) % P, k // 9


def test_doubling_equals_the_parent_formula(lib):
    rng = random.Random(41)
    r, o = U27(), U27()
    for it in range(200):
        pt = rnd_point(rng)
        p = U27(*wpoint(rng, pt, it % 3))
        lib.s_dbl_neg(r, p, 0)
        lib.s_dbl_neg(o, p, 1)
        same_field_elements(list(r), list(o), 3)
        assert w_affine(list(r)) == ec_neg(ec_mul(2, pt))
        for k in (0, 9, 18):
            check_mag1(list(r)[k:k + 9])


def test_doubling_at_the_largest_limbs(lib):
    """not a curve point: the formulas are polynomial identities, so the two forms still agree"""
    r, o = U27(), U27()
    w2 = [2 * x for x in prod_max()]
    for p in (prod_max() + w2 + prod_max(), [0] * 27, prod_max() + [0] * 9 + prod_max()):
        lib.s_dbl_neg(r, U27(*p), 0)
        lib.s_dbl_neg(o, U27(*p), 1)
        same_field_elements(list(r), list(o), 3)
        for k in (0, 9, 18):
            check_mag1(list(r)[k:k + 9])


def test_mixed_add_equals_the_parent_formula(lib):
    rng = random.Random(42)
    r, o = U45(), U45()
    for it in range(200):
        p, q = rnd_point(rng), rnd_point(rng)
        if it % 10 == 7:
            q = p              # H = rr = 0: the core's outputs are still the same polynomials
        elif it % 10 == 8:
            q = ec_neg(p)      # H = 0
        pl, ql = U27(*wpoint(rng, p, it % 3)), U18(*qlimbs(rng, q, it % 2))
        lib.s_add_ge_core(r, pl, ql, 0)
        lib.s_add_ge_core(o, pl, ql, 1)
        same_field_elements(list(r), list(o), 5)
        check_mag1(list(r)[0:9])
        check_w2(list(r)[9:18])
        for k in (18, 27, 36):
            check_mag1(list(r)[k:k + 9])
        if it % 10 == 7:
            assert val(list(r)[27:36]) % P == 0 and val(list(r)[36:45]) % P == 0
        elif it % 10 == 8:
            assert val(list(r)[27:36]) % P == 0 and val(list(r)[36:45]) % P != 0
        else:
            assert w_affine(list(r)[:27]) == ec_add(p, q)


def test_mixed_add_at_the_largest_limbs(lib):
    r, o = U45(), U45()
    w2 = [2 * x for x in prod_max()]
    q2 = limbs_at(2) + limbs_at(2)
    for p, q in ((prod_max() + w2 + prod_max(), q2), ([0] * 27, q2), (prod_max() + w2 + prod_max(), [0] * 18)):
        lib.s_add_ge_core(r, U27(*p), U18(*q), 0)
        lib.s_add_ge_core(o, U27(*p), U18(*q), 1)
        same_field_elements(list(r), list(o), 5)
        check_mag1(list(r)[0:9])
        check_w2(list(r)[9:18])
        for k in (18, 27, 36):
            check_mag1(list(r)[k:k + 9])


def test_mixed_add_exceptional_cases(lib):
    """the whole gejw_add_ge on the rewired core: p == infinity, p == q (the doubling), p == -q"""
    rng = random.Random(43)
    r = U27()
    for it in range(12):
        p, q = rnd_point(rng), rnd_point(rng)
        assert lib.s_add_ge(r, U27(*wpoint(rng, p, it % 3)), 1, U18(*qlimbs(rng, q, it % 2))) == 0
        assert w_affine(list(r)) == q
        assert lib.s_add_ge(r, U27(*wpoint(rng, p, it % 3)), 0, U18(*qlimbs(rng, p, it % 2))) == 0
        assert w_affine(list(r)) == ec_mul(2, p)
        check_mag1(list(r)[0:9])
        assert all(x < 2**30 for x in list(r)[9:18])
        check_mag1(list(r)[18:27])
        assert lib.s_add_ge(r, U27(*wpoint(rng, p, it % 3)), 0, U18(*qlimbs(rng, ec_neg(p), it % 2))) == 1
        assert lib.s_add_ge(r, U27(*wpoint(rng, p, it % 3)), 0, U18(*qlimbs(rng, q, it % 2))) == 0
        assert w_affine(list(r)) == ec_add(p, q)


def test_first_add_equals_the_parent_formula(lib):
    """gejw_add_ge_z1: p affine in the W convention (X1 at magnitude 1, W1 <= 2; Z not read)"""
    rng = random.Random(44)
    r, o = U27(), U27()
    for it in range(200):
        p, q = rnd_point(rng), rnd_point(rng)
        w = from_int(2 * p[1] % P) if it % 2 else [2 * x for x in from_int(p[1])]
        pl, ql = U27(*(from_int(p[0]) + w + from_int(1))), U18(*qlimbs(rng, q, it % 2))
        lib.s_add_ge_z1(r, pl, ql, 0)
        lib.s_add_ge_z1(o, pl, ql, 1)
        same_field_elements(list(r), list(o), 3)
        assert w_affine(list(r)) == ec_add(p, q)
        check_mag1(list(r)[0:9])
        check_w2(list(r)[9:18])
        check_mag1(list(r)[18:27])


def test_co_z_steps_equal_the_parent_formulas(lib):
    """ge9_dblu from an affine R, then ge9_zaddu on the co-Z pair it returns, chained as the table does"""
    rng = random.Random(45)
    r, o = U45(), U45()
    for it in range(100):
        R = rnd_point(rng)
        x, y = U9(*from_int(R[0])), U9(*from_int(R[1]))
        lib.s_dblu(r, x, y, 0)
        lib.s_dblu(o, x, y, 1)
        same_field_elements(list(r), list(o), 5)
        d, rp, z = list(r)[0:18], list(r)[18:36], val(list(r)[36:45]) % P
        zi = pow(z, -1, P)
        aff = lambda l: (val(l[0:9]) * zi * zi % P, val(l[9:18]) * zi**3 % P)
        assert aff(d) == ec_mul(2, R) and aff(rp) == R
        for k in (0, 9, 18, 27):
            check_mag1(list(r)[k:k + 9])
        for step in range(3):  # 3R = R' + D, then 5R, 7R: p1 = the running sum's co-Z partner D
            p1, p2 = U18(*d), U18(*rp)
            lib.s_zaddu(r, p1, p2, 0)
            lib.s_zaddu(o, p1, p2, 1)
            same_field_elements(list(r), list(o), 5)
            for k in (0, 9, 18, 27, 36):
                check_mag1(list(r)[k:k + 9])
            z = z * val(list(r)[36:45]) % P
            zi = pow(z, -1, P)
            s, d = list(r)[0:18], list(r)[18:36]
            assert aff(s) == ec_mul(3 + 2 * step, R) and aff(d) == ec_mul(2, R)
            rp = s
