"""Generates tests/golden/bn256_g1.json: fixtures of the bn256Add / bn256ScalarMul precompiles (run in
the build container, where /root/reference exists; the tests only read the JSON).

  add        the 16 bn256AddTests rows of the reference's own tests, copied as data
             (core/vm/contracts_test.go:119-185; the 18 bn256ScalarMulTests rows are in bn256.json)
  generated  seeded cases whose expectations come from the CPU oracle (oracle.bn256_g1_mul, pinned by
             tests/test_oracle.py against the reference's scalar-mul vectors):
             mul  k * P for P = s G, k uniform over 256 bits (and a few structured k)
             add  a G + b G, expected (a + b mod r) G, with a = b and a + b = 0 (mod r) mixed in;
                  the scalars are kept so a test can re-derive the expectation with its own model

    python tests/golden/make_bn256_g1.py
"""
from __future__ import annotations

import json
import os
import random
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
SEED = 608


def precompiled_tests(var):
    """(input, expected, name, line) rows of a precompiledTest table in core/vm/contracts_test.go"""
    src = open(os.path.join(REF, "core/vm/contracts_test.go")).read()
    i = src.index("var " + var)
    j = src.index("\n}\n", i)
    rows = []
    for m in re.finditer(r'input:\s*"([0-9a-f]*)",\s*expected:\s*"([0-9a-f]*)",\s*name:\s*"([^"]*)"', src[i:j]):
        rows.append((m.group(1), m.group(2), m.group(3), src[:i + m.start()].count("\n") + 1))
    return rows


def main():
    add = [{"input": a, "expected": e, "name": n, "source": f"core/vm/contracts_test.go:{ln}"}
           for a, e, n, ln in precompiled_tests("bn256AddTests")]
    assert len(add) == 16, len(add)
    rng = random.Random(SEED)
    gmul = []
    ks = [rng.getrandbits(256) for _ in range(24)] + [rng.getrandbits(20), R - 1, R, R + 1, 2**256 - 1, 2**255]
    for k in ks:
        s = rng.randrange(1, R)
        pt = O.bn256_g1_mul(s)
        gmul.append({"point_scalar": hex(s), "point": pt.hex(), "k": hex(k), "expected": O.bn256_g1_mul(k, pt).hex()})
    gadd = []
    for i in range(24):
        a = rng.randrange(1, R)
        b = a if i % 6 == 4 else (R - a) if i % 6 == 5 else rng.randrange(1, R)
        gadd.append({"a": hex(a), "b": hex(b), "input": (O.bn256_g1_mul(a) + O.bn256_g1_mul(b)).hex(),
                     "expected": O.bn256_g1_mul((a + b) % R).hex()})
    with open(os.path.join(OUT, "bn256_g1.json"), "w") as f:
        json.dump({"add": add, "generated": {"seed": SEED, "mul": gmul, "add": gadd}}, f, indent=1, sort_keys=True)
    print("wrote bn256_g1.json")


if __name__ == "__main__":
    main()
