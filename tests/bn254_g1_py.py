"""TEST INFRASTRUCTURE — a pure-Python affine model of BN254 G1 and of the bn256Add / bn256ScalarMul
precompiles (core/vm/contracts.go:274-312, crypto/bn256/cloudflare/bn256.go:62-158), independent of
the C oracle and of the code under test.  None is the point at infinity."""
from __future__ import annotations

from bn254_py import P, R, g1_on_curve

G = (1, 2)
# the endomorphism (x, y) -> (BETA x, y) = LAMBDA (x, y): BETA is the reference's
# xiTo2PSquaredMinus2Over3 (constants.go), LAMBDA the matching cube root of unity mod r
BETA = 0x30644e72e131a0295e6dd9e7e0acccb0c28f069fbb966e3de4bd44e5607cfd48
LAMBDA = 0x30644e72e131a029048b6e193fd84104cc37a73fec2bc5e9b8ca0b2d36636f23


def g1_add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    (x1, y1), (x2, y2) = p, q
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return None
        lam = 3 * x1 * x1 * pow(2 * y1, -1, P) % P
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return (x3, (lam * (x1 - x3) - y1) % P)


def g1_mul(p, k):
    r = None
    while k:
        if k & 1:
            r = g1_add(r, p)
        p = g1_add(p, p)
        k >>= 1
    return r


def g1_neg(p):
    return None if p is None else (p[0], (P - p[1]) % P)


def g1_encode(p) -> bytes:
    return bytes(64) if p is None else p[0].to_bytes(32, "big") + p[1].to_bytes(32, "big")


class Malformed(ValueError):
    pass


def g1_decode(b: bytes):
    """G1.Unmarshal (bn256.go:120-158)"""
    x, y = int.from_bytes(b[:32], "big"), int.from_bytes(b[32:64], "big")
    if x >= P or y >= P:
        raise Malformed("coordinate exceeds modulus")
    if x == 0 and y == 0:
        return None
    if not g1_on_curve(x, y):
        raise Malformed("not on curve")
    return (x, y)


def run_add(inp: bytes):
    """bn256Add.Run: 64 bytes, or None where the reference returns the unmarshal error"""
    b = bytes(inp).ljust(128, b"\0")[:128]
    try:
        return g1_encode(g1_add(g1_decode(b[:64]), g1_decode(b[64:])))
    except Malformed:
        return None


def run_mul(inp: bytes):
    b = bytes(inp).ljust(96, b"\0")[:96]
    try:
        return g1_encode(g1_mul(g1_decode(b[:64]), int.from_bytes(b[64:], "big") % R))
    except Malformed:
        return None


# the scalars every multiplication test covers (issue list), for the endomorphism above
EDGE_SCALARS = list(range(17)) + [R - 1, R, R + 1, 2 * R, 2**256 - 1, 2**255, 2**254, 2**253, 2**128, 2**127, 2**64,
                                  (R - 1) // 2, LAMBDA, LAMBDA - 1, LAMBDA + 1]
