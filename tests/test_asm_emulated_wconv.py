"""The two fused products of the W-convention doubling (tools/gen_fe9_asm.py: fe9_dot_ms_full,
r = a b + c^2, and fe9_sqr3_full, r = 3 a^2), column form 3, executed instruction by instruction on
the CPU by the emulator of tests/test_asm_emulated.py (every 64-bit multiply-add, shift-add and
32-bit shift is checked not to wrap), against Python integers: at random, at the extreme limbs
their preconditions admit, and at the exact operands gejw_dbl_neg and gejw_add_ge_core
(secp256k1_fe9.cuh) feed them and their neighbours, W at magnitude 2 included."""
import random

import pytest

from test_asm_emulated import M32, _q_consts, check_weak, fe9_case, fe9_lines, limbs_val, run_fe9  # puts tools/ on the path

import gen_fe9_asm  # noqa: E402

FORM = 3

# a product's output at its largest limbs (limb 2 up to 2^29 + 2^24, limb 8 < 2^24)
PROD = [(1 << 29) - 1] * 9
PROD[2] = (1 << 29) + (1 << 24) - 1
PROD[8] = (1 << 24) - 1


def dot_ms_want(a, b, c):
    return limbs_val(a) * limbs_val(b) + limbs_val(c) ** 2


def run_dot_ms(lines, a, b, c):
    d = [x << 1 for x in c]
    assert max(d) <= M32
    return run_fe9(lines, a, b, c, d)


def run_sqr3(lines, a):
    a3 = [3 * x for x in a]
    a6 = [6 * x for x in a]
    assert max(a6) <= M32
    return run_fe9(lines, a, a6, a3)


@pytest.mark.parametrize("m", [(1, 6, 1), (6, 1, 1), (1.04, 5.6, 1.04), (1, 3, 2), (1.5, 1.5, 2.17), (1, 1, 2.44)])
def test_fe9_dot_ms_asm(m):
    """a*b + c^2 with one reduction at m_a m_b + m_c^2 <= 7"""
    ma, mb, mc = m
    assert ma * mb + mc * mc <= 7.0
    rng = random.Random(int(sum(m) * 1000))
    lines = fe9_lines(FORM, gen_fe9_asm.DOT_MS_TERMS)
    for it in range(150):
        a, b = fe9_case(rng, ma, mb, extreme=(it == 0))
        c, _ = fe9_case(rng, mc, 1, extreme=(it == 0))
        check_weak(run_dot_ms(lines, a, b, c), dot_ms_want(a, b, c))


def test_fe9_dot_ms_asm_at_the_doubling_operands():
    """gejw_dbl_neg's -W3 = E 2(X3 - D) + B B at the largest limbs: E, B, X3 product outputs,
    2(X3 - D) = 2 (X3 + Q_1 - D) (limb 8 near 2^31, far above a product output's 2^24): 1*6 + 1*1"""
    Q = _q_consts()
    t = [2 * (PROD[i] + Q[1][i]) for i in range(9)]    # D = 0
    lines = fe9_lines(FORM, gen_fe9_asm.DOT_MS_TERMS)
    check_weak(run_dot_ms(lines, PROD, t, PROD), dot_ms_want(PROD, t, PROD))
    rng = random.Random(17)
    for _ in range(200):
        a = [rng.randrange(x + 1) for x in PROD]
        b = [rng.randrange(x + 1) for x in t]
        c = [rng.randrange(x + 1) for x in PROD]
        check_weak(run_dot_ms(lines, a, b, c), dot_ms_want(a, b, c))


@pytest.mark.parametrize("ma", [1, 1.04, 1.33])
def test_fe9_sqr3_asm(ma):
    """3 a^2 on (a, 6a, 3a), m_a <= 1.33 (6a < 2^32)"""
    rng = random.Random(int(ma * 1000) + 3)
    lines = fe9_lines(FORM, gen_fe9_asm.SQR3_TERMS)
    for it in range(150):
        a, _ = fe9_case(rng, ma, 1, extreme=(it == 0))
        check_weak(run_sqr3(lines, a), 3 * limbs_val(a) ** 2)


def test_fe9_sqr3_asm_at_the_doubling_operand():
    """E = 3 X^2 with X a product's output (out of the doubling's fe9_sqr_add or the mixed add's)"""
    lines = fe9_lines(FORM, gen_fe9_asm.SQR3_TERMS)
    check_weak(run_sqr3(lines, PROD), 3 * limbs_val(PROD) ** 2)


def _w_mag2_cases():
    """W as its two producers hand it over: a product's output doubled limb-wise (gejw_add_ge_core)
    and Q_1 minus a product's output (gejw_dbl, the rare p == q case: limb 8 near 2^30)"""
    Q = _q_consts()
    return [[2 * x for x in PROD], list(Q[1])]


@pytest.mark.parametrize("wi", [0, 1])
def test_w_at_magnitude_2_into_its_consumers(wi):
    """W at magnitude 2 at its largest limbs into every product that reads it: the mixed add's
    Y3 = rr (V - X3) + W1 (-J) (1*3 + 2*2 = 7, the bound itself), the doubling's W^2 and W Z"""
    Q = _q_consts()
    W = _w_mag2_cases()[wi]
    t = [PROD[i] + Q[1][i] for i in range(9)]          # V - X3 with X3 = 0
    nj = list(Q[1])                                    # -J with J = 0
    dot = fe9_lines(FORM, gen_fe9_asm.DOT_TERMS)
    check_weak(run_fe9(dot, PROD, t, W, nj), limbs_val(PROD) * limbs_val(t) + limbs_val(W) * limbs_val(nj))
    sqr = fe9_lines(FORM, gen_fe9_asm.SQR_TERMS)
    check_weak(run_fe9(sqr, W, [x << 1 for x in W]), limbs_val(W) ** 2)
    mul = fe9_lines(FORM, gen_fe9_asm.MUL_TERMS)
    check_weak(run_fe9(mul, W, PROD), limbs_val(W) * limbs_val(PROD))
    rng = random.Random(23 + wi)
    for _ in range(100):
        a = [rng.randrange(x + 1) for x in PROD]
        b = [rng.randrange(x + 1) for x in t]
        c = [rng.randrange(x + 1) for x in W]
        d = [rng.randrange(x + 1) for x in nj]
        check_weak(run_fe9(dot, a, b, c, d), limbs_val(a) * limbs_val(b) + limbs_val(c) * limbs_val(d))
