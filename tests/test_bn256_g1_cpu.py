"""CPU tests of the bn256Add / bn256ScalarMul feature: the boundary (header, exports, precompile
classes), the fixtures against a pure-Python model and the oracle, and the scalar recoding plus the
whole per-item functions of geth-sharding_amd/csrc/bn_g1.cuh compiled for the host
(tests/native/bn_g1_recode_host.cpp) against Python integers.  No GPU."""
import ctypes
import os
import random
import re

import pytest

import bn254_g1_py as M
from bn254_py import P, R
from conftest import ROOT, golden

NEW = ["gsv_bn256_add_batch", "gsv_bn256_add_batch_dev", "gsv_bn256_scalar_mul_batch",
       "gsv_bn256_scalar_mul_batch_dev"]


def test_boundary_declared_exported_and_mirrored():
    txt = open(os.path.join(ROOT, "include", "gsv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from gsv import _lib, bn256
    L = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, code), s
        assert hasattr(L, s), s
    assert int(re.search(r"#define GSV_K_BN_G1 (\d+)", txt).group(1)) == _lib.K_BN_G1 == 11
    assert int(re.search(r"#define GSV_K_COUNT (\d+)", txt).group(1)) == 12
    assert int(re.search(r"#define GSV_ABI_VERSION (\d+)", txt).group(1)) == 2
    assert bn256.Bn256Add().RequiredGas(b"") == 500
    assert bn256.Bn256ScalarMul().RequiredGas(b"") == 40000
    # argument checks precede every HIP call
    assert L.gsv_bn256_add_batch(None, None, None, 1, None, None) == _lib.E_INVALID_ARG
    assert L.gsv_bn256_scalar_mul_batch_dev(None, None, 1, None, None, None) == _lib.E_INVALID_ARG


# ---------------------------------------------------------------- fixtures
def test_model_constants():
    assert pow(M.BETA, 3, P) == 1 and M.BETA != 1 and pow(M.LAMBDA, 3, R) == 1 and M.LAMBDA != 1
    assert M.g1_mul(M.G, M.LAMBDA) == (M.BETA * M.G[0] % P, M.G[1])
    assert M.g1_mul(M.G, R) is None


def test_reference_vectors_against_model():
    add = golden("bn256_g1.json")["add"]
    mul = golden("bn256.json")["scalar_mul"]
    assert len(add) == 16 and len(mul) == 18
    for r in add:
        assert M.run_add(bytes.fromhex(r["input"])).hex() == r["expected"], r["name"]
    for r in mul:
        assert M.run_mul(bytes.fromhex(r["input"])).hex() == r["expected"], r["name"]


def test_generated_cases_against_model_and_oracle(oracle):
    g = golden("bn256_g1.json")["generated"]
    assert len(g["mul"]) >= 24 and len(g["add"]) >= 24
    for c in g["mul"][::3]:  # the model's double-and-add in Python integers: a third of the rows
        pt, k = bytes.fromhex(c["point"]), int(c["k"], 16)
        assert M.g1_encode(M.g1_mul(M.G, int(c["point_scalar"], 16))) == pt
        assert M.run_mul(pt + k.to_bytes(32, "big")).hex() == c["expected"]
    for c in g["mul"]:
        pt, k = bytes.fromhex(c["point"]), int(c["k"], 16)
        assert oracle.bn256_g1_mul(k, pt).hex() == c["expected"]
    kinds = set()
    for c in g["add"]:
        a, b = int(c["a"], 16), int(c["b"], 16)
        kinds.add("dbl" if a == b else "inf" if (a + b) % R == 0 else "gen")
        inp = bytes.fromhex(c["input"])
        assert inp == oracle.bn256_g1_mul(a) + oracle.bn256_g1_mul(b)
        assert oracle.bn256_g1_mul((a + b) % R).hex() == c["expected"]
        assert M.run_add(inp).hex() == c["expected"]  # add(aG, bG) == (a + b mod r) G by the model's law
    assert kinds == {"dbl", "inf", "gen"}


# ---------------------------------------------------------------- host build of bn_g1.cuh
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    from conftest import build_native
    return build_native("bn_g1_recode_host.cpp", tmp_path_factory.mktemp("bng1") / "bn_g1_host.so")


U8W = ctypes.c_uint32 * 8


def words(k):
    return U8W(*[(k >> (32 * i)) & 0xFFFFFFFF for i in range(8)])


# the lattice of bn_g1.cuh, restated: (a, b) with a + b LAMBDA = 0 (mod r)
V1 = (147946756881789319000765030803803410728, -9931322734385697763)
V2 = (9931322734385697763, 147946756881789319010696353538189108491)


def split_py(k):
    """the rounding split in Python integers (what g1_glv_split computes in words)"""
    g1 = (V2[1] << 288) // R + (1 if ((V2[1] << 289) // R) & 1 else 0)   # round(2^288 b2 / r)
    g2 = (-V1[1] << 288) // R + (1 if ((-V1[1] << 289) // R) & 1 else 0)  # round(2^288 (-b1) / r)
    c1 = (k * g1 + (1 << 287)) >> 288
    c2 = (k * g2 + (1 << 287)) >> 288
    return k - c1 * V1[0] - c2 * V2[0], -c1 * V1[1] - c2 * V2[1]


def test_recoding(host):
    assert (V1[0] + V1[1] * M.LAMBDA) % R == 0 and (V2[0] + V2[1] * M.LAMBDA) % R == 0
    assert V1[0] * V2[1] - V2[0] * V1[1] == R
    rng = random.Random(1207)
    ks = M.EDGE_SCALARS + [rng.getrandbits(256) for _ in range(10000)]
    out = (ctypes.c_uint32 * 12)()
    dig = (ctypes.c_uint8 * 128)()
    bits = (ctypes.c_uint8 * 256)()
    for k in ks:
        host.h_g1_split(out, words(k))
        m1 = sum(int(out[i]) << (32 * i) for i in range(5))
        m2 = sum(int(out[6 + i]) << (32 * i) for i in range(5))
        k1 = -m1 if out[5] else m1
        k2 = -m2 if out[11] else m2
        assert (k1, k2) == split_py(k), hex(k)
        assert (k1 + k2 * M.LAMBDA - k) % R == 0, hex(k)          # reconstructs k mod r
        assert m1 < 2**127 and m2 < 2**127, hex(k)                 # the loop takes 128 bits
        host.h_g1_digits(dig, words(k))
        for b in range(128):
            want = ((m1 >> (127 - b)) & 1) | (((m2 >> (127 - b)) & 1) << 1)
            assert dig[b] == want, (hex(k), b)
    for k in M.EDGE_SCALARS + [rng.getrandbits(256) for _ in range(200)]:
        host.h_g1_bits(bits, words(k))
        assert sum(int(bits[b]) << (255 - b) for b in range(256)) == k


def test_host_items_against_model(host):
    """the per-item functions the kernels run (decode, both multiplication forms, the complete
    addition, the one inversion, marshal) on the host, against the model"""
    rng = random.Random(99)
    out = ctypes.create_string_buffer(64)
    pt = M.g1_mul(M.G, rng.randrange(1, R))
    for p in (M.G, pt):
        for k in M.EDGE_SCALARS + [rng.getrandbits(256) for _ in range(12)]:
            inp = M.g1_encode(p) + k.to_bytes(32, "big")
            want = M.run_mul(inp)
            for bitserial in (0, 1):
                assert host.h_g1_mul(out, inp, bitserial) == 0 and out.raw == want, (hex(k), bitserial)
    assert host.h_g1_mul(out, bytes(64) + (5).to_bytes(32, "big"), 0) == 0 and out.raw == bytes(64)
    bad = [(1, 3), (0, 1), (P, 2), (1, P), (P + 1, 2), (2**256 - 1, 2)]
    for x, y in bad:
        enc = x.to_bytes(32, "big") + y.to_bytes(32, "big")
        assert host.h_g1_mul(out, enc + bytes(32), 0) == 9 and out.raw == bytes(64)
        assert host.h_g1_add(out, enc + M.g1_encode(pt)) == 9 and out.raw == bytes(64)
        assert host.h_g1_add(out, M.g1_encode(pt) + enc) == 9 and out.raw == bytes(64)
    for a, b in ((pt, None), (None, pt), (None, None), (pt, pt), (pt, M.g1_neg(pt)), (M.G, pt), (pt, M.G)):
        assert host.h_g1_add(out, M.g1_encode(a) + M.g1_encode(b)) == 0
        assert out.raw == M.g1_encode(M.g1_add(a, b))
