"""RIPEMD-160 in pure Python: the suite's oracle for csrc/ripemd160_dev.cuh (hashlib here has no ripemd160).

Written from the specification (Dobbertin, Bosselaers, Preneel: "RIPEMD-160: a strengthened version of
RIPEMD", 1996).  Two lines of 80 steps over the same 16 little-endian message words.  The word orders come
from two permutations: rho, and pi(i) = 9i + 5 mod 16; the left line reads the words in the orders
id, rho, rho^2, rho^3, rho^4 and the right line in pi, rho pi, ... .  The rotate amount of a step depends on
its round and on the word it reads.  The additive constants are floor(2^30 sqrt(p)) on the left and
floor(2^30 cbrt(p)) on the right for p = 2, 3, 5, 7, and 0 in the left line's first and the right line's last
round.  The fixture tests/golden/md_hashes.json pins it to digests made with another implementation.
"""
import struct

M32 = 0xFFFFFFFF

RHO = [7, 4, 13, 1, 10, 6, 15, 3, 12, 0, 9, 5, 2, 14, 11, 8]
PI = [(9 * i + 5) % 16 for i in range(16)]
# rotate amounts: SHIFT[round][message word]
SHIFT = [[11, 14, 15, 12, 5, 8, 7, 9, 11, 13, 14, 15, 6, 7, 9, 8],
         [12, 13, 11, 15, 6, 9, 9, 7, 12, 15, 11, 13, 7, 8, 7, 7],
         [13, 15, 14, 11, 7, 7, 6, 8, 13, 14, 13, 12, 5, 5, 6, 9],
         [14, 11, 12, 14, 8, 6, 5, 5, 15, 12, 15, 14, 9, 9, 8, 6],
         [15, 12, 13, 13, 9, 5, 8, 6, 14, 11, 12, 11, 8, 6, 5, 5]]


def _orders(first):
    out, cur = [], list(first)
    for _ in range(5):
        out += cur
        cur = [RHO[i] for i in cur]
    return out


def _iroot(x, k):
    lo, hi = 0, 1 << (x.bit_length() // k + 1)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if mid ** k <= x:
            lo = mid
        else:
            hi = mid - 1
    return lo


RL = _orders(range(16))          # word read by step j of the left line
RR = _orders(PI)                 # ... of the right line
SL = [SHIFT[j // 16][RL[j]] for j in range(80)]
SR = [SHIFT[j // 16][RR[j]] for j in range(80)]
KL = [0] + [_iroot(p << 60, 2) for p in (2, 3, 5, 7)]   # floor(2^30 sqrt(p))
KR = [_iroot(p << 90, 3) for p in (2, 3, 5, 7)] + [0]   # floor(2^30 cbrt(p))
IV = [0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0]

F = [lambda x, y, z: x ^ y ^ z,
     lambda x, y, z: (x & y) | (~x & z),
     lambda x, y, z: (x | ~y) ^ z,
     lambda x, y, z: (x & z) | (y & ~z),
     lambda x, y, z: x ^ (y | ~z)]


def rol(x, s):
    return ((x << s) | (x >> (32 - s))) & M32


def compress(h, block):
    x = struct.unpack("<16I", block)
    a, b, c, d, e = h
    ar, br, cr, dr, er = h
    for j in range(80):
        t = (rol((a + (F[j // 16](b, c, d) & M32) + x[RL[j]] + KL[j // 16]) & M32, SL[j]) + e) & M32
        a, e, d, c, b = e, d, rol(c, 10), b, t
        t = (rol((ar + (F[4 - j // 16](br, cr, dr) & M32) + x[RR[j]] + KR[j // 16]) & M32, SR[j]) + er) & M32
        ar, er, dr, cr, br = er, dr, rol(cr, 10), br, t
    return [(h[1] + c + dr) & M32, (h[2] + d + er) & M32, (h[3] + e + ar) & M32, (h[4] + a + br) & M32,
            (h[0] + b + cr) & M32]


def pad(n):
    """the Merkle-Damgard padding of an n-byte message: 0x80, zeros, the bit length as 64 little-endian bits"""
    return b"\x80" + bytes((55 - n) % 64) + struct.pack("<Q", (8 * n) & 0xFFFFFFFFFFFFFFFF)


def ripemd160(msg: bytes) -> bytes:
    msg = bytes(msg)
    m = msg + pad(len(msg))
    h = list(IV)
    for i in range(0, len(m), 64):
        h = compress(h, m[i:i + 64])
    return struct.pack("<5I", *h)


def precompile_row(msg: bytes) -> bytes:
    """common.LeftPadBytes(digest, 32): what the ripemd160hash precompile returns (core/vm/contracts.go:129-133)"""
    return bytes(12) + ripemd160(msg)


def long_message(n: int) -> bytes:
    """the fixture's long message: byte i is (i^2 + 7i + (i >> 8)) mod 256"""
    return bytes((i * i + 7 * i + (i >> 8)) & 0xFF for i in range(n))
