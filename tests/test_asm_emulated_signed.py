"""The subtrahend statements of tools/gen_fe9_asm.py (full_lines3s: fe9_mul_sub_full, r = a b - c, and
the fe9_sqr_sub* family, r = a^2 - c - k d), executed instruction by instruction on the CPU.

The emulator of tests/test_asm_emulated.py gains the two signed instructions (v_mad_i64_i32, the
arithmetic 64-bit shift) and reads the low chain D = v[4:5] as a SIGNED 64-bit value: every
multiply-add into it and every value shifted out of it is asserted to lie in [-2^63, 2^63), and what
leaves it for T (the part at and above 2^256) is asserted non-negative.  The high columns keep the
base emulator's unsigned checks.  Inputs: all limbs at their magnitude maxima, subtrahends at 2^31 - 1
and at 0, product operands at 0 (the most negative chains), and 2,000 random inputs; results against
Python integers mod p, outputs within a product's output bounds."""
import random

import pytest

from test_asm_emulated import M32, M64, Machine, check_weak, fe9_case, limbs_val  # puts tools/ on the path

import gen_fe9_asm  # noqa: E402

S63 = 1 << 63
DPAIR = "v[4:5]"


def s32(x):
    return x - (1 << 32) if x & (1 << 31) else x


def s64(x):
    return x - (1 << 64) if x & S63 else x


class SignedMachine(Machine):
    """Machine + v_mad_i64_i32, v_ashrrev_i64, v_lshl_add_u32, and D as a signed accumulator"""

    def __init__(self, ops):
        super().__init__(ops)
        self.lowest = 0   # the most negative value D ever held

    def r64s(self, x):
        if x.startswith("%"):
            return s64(self.ops[int(x[1:])] & M64)   # a 64-bit SGPR constant
        return s64(self.r64(x))

    def w64s(self, x, val, ln):
        assert -S63 <= val < S63, f"signed 64-bit overflow in {ln}: {val}"
        self.lowest = min(self.lowest, val)
        self.w64(x, val & M64)

    def run(self, lines):
        for ln in lines:
            op, rest = ln.split(" ", 1)
            a = [t.strip() for t in rest.split(",")]
            if op == "v_mad_i64_i32":
                assert a[0] == DPAIR
                x = self.r32(a[2])
                assert x < (1 << 31), f"subtrahend limb is not a non-negative i32 in {ln}"
                self.w64s(a[0], s32(x) * int(a[3], 0) + self.r64s(a[4]), ln)
            elif op == "v_ashrrev_i64":
                assert a[0] == DPAIR and a[2] == DPAIR
                self.w64s(a[0], self.r64s(a[2]) >> int(a[1]), ln)
            elif op == "v_lshl_add_u32":
                res = (self.r32(a[1]) << int(a[2])) + self.r32(a[3])
                assert res <= M32, f"32-bit overflow in {ln}"
                self.w32(a[0], res)
            elif op == "v_mad_u64_u32" and a[4] == DPAIR:
                res = self.r32(a[2]) * self.r32(a[3]) + self.r64s(a[4])
                if a[0] == DPAIR:
                    self.w64s(a[0], res, ln)
                else:   # T: multiplied as an unsigned value afterwards
                    assert 0 <= res <= M64, f"T is negative or overflows in {ln}: {res}"
                    self.w64(a[0], res)
            else:
                super().run([ln])


def run_sub(terms, ks, a, b, subs):
    O = gen_fe9_asm.opnd3s(len(ks))
    ops = {O["a"] + i: a[i] for i in range(9)}
    ops.update({O["b"] + j: b[j] for j in range(9)})
    for n, s in enumerate(subs):
        ops.update({O[f"s{n}"] + j: s[j] for j in range(9)})
    ops.update({O["k31264"]: 31264, O["k256"]: 256, O["k977"]: 977, O["k8192"]: 8192,
                O["k250112"]: 8 * 31264, O["kbias"]: gen_fe9_asm.SUB_BIAS0 & M64})
    m = SignedMachine(ops)
    m.run(gen_fe9_asm.full_lines3s(terms, ks))
    return [m.ops[O["r"] + i] for i in range(9)], m.lowest


SUB_MAX = [(1 << 31) - 1] * 9
ZERO = [0] * 9
STATEMENTS = {"mul_sub": (gen_fe9_asm.MUL_TERMS, [1]), "sqr_sub2_k1": (gen_fe9_asm.SQR_TERMS, [1, 1]),
              "sqr_sub2_k2": (gen_fe9_asm.SQR_TERMS, [1, 2]), "sqr_sub1_k2": (gen_fe9_asm.SQR_TERMS, [2])}
# (m_a, m_b) at the statements' bound m_a m_b <= 3.5; squarings read the first only (m_a <= 1.87)
MAGS = {"mul_sub": [(1.04, 3.36), (3.36, 1.04), (2, 1.75), (1.87, 1.87)], "sqr": [(1.04, 0), (1.5, 0), (1.87, 0)]}


def operands(name, rng, ma, mb, extreme):
    a, b = fe9_case(rng, ma, mb or 1, extreme)
    if name != "mul_sub":
        b = [x << 1 for x in a]
        assert max(b) <= M32
    return a, b


def want(name, ks, a, b, subs):
    prod = limbs_val(a) * (limbs_val(b) if name == "mul_sub" else limbs_val(a))
    return prod - sum(k * limbs_val(s) for k, s in zip(ks, subs))


def sub_case(rng, n, kind):
    if kind == "max":
        return [list(SUB_MAX) for _ in range(n)]
    if kind == "zero":
        return [list(ZERO) for _ in range(n)]
    return [[rng.randrange(1 << 31) for _ in range(9)] for _ in range(n)]


@pytest.mark.parametrize("name", list(STATEMENTS))
def test_generated_text_matches_the_emulated_lines(name):
    """what the emulator runs is what fe9_asm.cuh holds"""
    import os
    terms, ks = STATEMENTS[name]
    body = "\\n\\t".join(gen_fe9_asm.full_lines3s(terms, ks))
    src = open(os.path.join(os.path.dirname(gen_fe9_asm.OUT), "fe9_asm.cuh")).read()
    assert f"fe9_{name}_full(" in src and body in src


@pytest.mark.parametrize("name", list(STATEMENTS))
def test_extremes(name):
    """limbs at their maxima against subtrahends at 2^31 - 1 and at 0, and product operands at 0
    against the largest subtrahends: the most positive and the most negative chains"""
    terms, ks = STATEMENTS[name]
    rng = random.Random(1)
    for (ma, mb) in MAGS["mul_sub" if name == "mul_sub" else "sqr"]:
        a, b = operands(name, rng, ma, mb, extreme=True)
        # the same with limb 8 as large as the others (a limb-wise difference: V + Q_1 - X3)
        a9 = [int(ma * (1 << 29)) - 1] * 9
        b9 = [int(mb * (1 << 29)) - 1] * 9 if name == "mul_sub" else [x << 1 for x in a9]
        for (x, y) in ((a, b), (a9, b9)):
            for kind in ("max", "zero"):
                subs = sub_case(rng, len(ks), kind)
                r, _ = run_sub(terms, ks, x, y, subs)
                check_weak(r, want(name, ks, x, y, subs))
    subs = sub_case(rng, len(ks), "max")
    r, lowest = run_sub(terms, ks, ZERO, ZERO, subs)
    check_weak(r, want(name, ks, ZERO, ZERO, subs))
    assert -(1 << 47) < lowest < 0          # the generator's stated lower bound; the chains did go negative
    r, _ = run_sub(terms, ks, ZERO, ZERO, sub_case(rng, len(ks), "zero"))
    check_weak(r, 0)


@pytest.mark.parametrize("name", list(STATEMENTS))
def test_random(name):
    """2,000 random inputs a statement, spread over its magnitudes, operands borrowed up to their limb
    bounds; one in eight with a zero product operand"""
    terms, ks = STATEMENTS[name]
    mags = MAGS["mul_sub" if name == "mul_sub" else "sqr"]
    rng = random.Random(len(name) * 31 + sum(ks))
    for it in range(2000):
        ma, mb = mags[it % len(mags)]
        a, b = operands(name, rng, ma, mb, extreme=False)
        if it % 8 == 7:
            a = list(ZERO)
            if name != "mul_sub":
                b = list(ZERO)
        subs = sub_case(rng, len(ks), "rnd")
        r, _ = run_sub(terms, ks, a, b, subs)
        check_weak(r, want(name, ks, a, b, subs))


def test_the_magnitude_2_square_does_not_fit():
    """why Z3 = (Z1 + H)^2 - Z1^2 - H^2 keeps the unsigned addend form: at magnitude 2 the squaring's
    column 7 passes 2^63 and the emulator refuses the signed chain"""
    terms, ks = STATEMENTS["sqr_sub2_k1"]
    a = [(2 << 29) - 1] * 8 + [(2 << 24) - 1]
    with pytest.raises(AssertionError, match="signed 64-bit overflow"):
        run_sub(terms, ks, a, [x << 1 for x in a], [list(ZERO), list(ZERO)])
