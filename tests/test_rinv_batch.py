"""Host build of the batched r inversion (geth-sharding_amd/csrc/secp256k1_rinv.cuh: prefix products,
ONE safegcd inversion, back-substitution; r == 0 and r >= n enter the product as 1) against Python's
pow(x, -1, n).  The routine is the one k_rinv_batch runs on the GPU; only sc_mul differs (the header's
plain C++ product here, inline asm there), so the host product is checked on its own as well.  CPU-only."""
import ctypes
import os
import random
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
W8 = ctypes.c_uint32 * 8


def rinv_k():
    """RINV_K as the library is built by default (gsv_internal.h)"""
    text = open(os.path.join(HERE, "..", "geth-sharding_amd", "csrc", "gsv_internal.h")).read()
    (k,) = re.findall(r"^#define GSV_RINV_K (\d+)$", text, re.M)
    return int(k)


K = rinv_k()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    from conftest import build_native
    return build_native("rinv_host.cpp", tmp_path_factory.mktemp("rinv") / "rinv_host.so")


def words(x):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def run(lib, xs):
    n = len(xs)
    A = ctypes.c_uint32 * (8 * n)
    slot = A(*([0xFFFFFFFF] * (8 * n)))
    lib.h_batch_inverse(slot, A(*[w for x in xs for w in words(x)]), n)
    return [sum(slot[8 * i + k] << (32 * k) for k in range(8)) for i in range(n)]


def check(lib, xs):
    got = run(lib, xs)
    for i, (x, g) in enumerate(zip(xs, got)):
        if 0 < x < N:
            assert g == pow(x, -1, N), (i, hex(x), hex(g))
        else:
            assert g < N, (i, hex(x), hex(g))  # substituted by 1: some reduced value, never used


SIZES = sorted({1, 2, K - 1, K})
SPECIAL = [1, 2, N - 1, 2**255, N - 2**128]
BAD = [0, N, N + 1, 2**256 - 1]


def test_k_is_what_the_shapes_assume():
    assert K >= 3


def test_host_sc_mul(lib):
    rng = random.Random(1)
    vals = SPECIAL + [N - 2, 3, 2**128, 2**129 - 1] + [rng.randrange(N) for _ in range(300)]
    out = W8()
    for a in vals:
        for b in (vals[rng.randrange(len(vals))], N - 1, 1, a):
            lib.h_sc_mul(out, W8(*words(a)), W8(*words(b)))
            assert sum(v << (32 * i) for i, v in enumerate(out)) == a * b % N


def test_operand_substitution(lib):
    for x in BAD + SPECIAL + [N - 1, N - 2]:
        w = W8(*words(x))
        lib.h_rinv_operand(w)
        assert sum(v << (32 * i) for i, v in enumerate(w)) == (x if 0 < x < N else 1)


@pytest.mark.parametrize("size", SIZES)
def test_special_values_at_every_position(lib, size):
    rng = random.Random(100 + size)
    for v in SPECIAL:
        for pos in sorted({0, size // 2, size - 1}):
            xs = [rng.randrange(1, N) for _ in range(size)]
            xs[pos] = v
            check(lib, xs)
    check(lib, [SPECIAL[i % len(SPECIAL)] for i in range(size)])  # nothing but special values


@pytest.mark.parametrize("size", SIZES)
def test_mixed_bit_lengths(lib, size):
    rng = random.Random(200 + size)
    for _ in range(40):
        xs = [max(1, rng.getrandbits(rng.choice([1, 8, 31, 32, 33, 64, 127, 128, 129, 200, 255, 256])) % N)
              for _ in range(size)]
        check(lib, xs)


@pytest.mark.parametrize("size", SIZES)
def test_zero_and_overflow_members(lib, size):
    """r == 0 and r >= n first, in the middle and last: the others' inverses stay exact, the
    substituted outputs are reduced"""
    rng = random.Random(300 + size)
    for bad in BAD:
        for pos in sorted({0, size // 2, size - 1}):
            xs = [rng.randrange(1, N) for _ in range(size)]
            xs[pos] = bad
            check(lib, xs)
    check(lib, [BAD[i % len(BAD)] for i in range(size)])  # every member substituted
    if size >= 3:
        xs = [rng.randrange(1, N) for _ in range(size)]
        xs[0], xs[size // 2], xs[-1] = 0, N, 2**256 - 1
        check(lib, xs)


def test_random_groups(lib):
    rng = random.Random(400)
    for _ in range(200):
        check(lib, [rng.randrange(1, N) for _ in range(rng.randrange(1, K + 1))])
