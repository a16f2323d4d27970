"""ECDSA verification with a known key and public-key parsing in Python integers: the semantics
gsv_ecdsa_verify_batch and gsv_pubkey_parse_batch pin (include/gsv.h), restated from the reference's cgo
path (libsecp256k1's ecdsa_signature_parse_compact, eckey_pubkey_parse, ecdsa_sig_verify).

Curve arithmetic, lift_x and the constants come from secp_glv_model (which reads them from the device
headers)."""
import random

import secp_glv_model as M

N, P, G, HALF_N = M.N, M.P, M.G, M.HALF_N

BAD_LENGTHS = (0, 32, 34, 64, 66)


def be32(x):
    return int(x).to_bytes(32, "big")


def on_curve(x, y):
    return (y * y - x * x * x - 7) % P == 0


def parse_pubkey(pub: bytes):
    """eckey_pubkey_parse: the affine point, or None"""
    pub = bytes(pub)
    if len(pub) == 33 and pub[0] in (2, 3):
        return M.lift_x(int.from_bytes(pub[1:], "big"), pub[0] & 1)
    if len(pub) == 65 and pub[0] in (4, 6, 7):
        x, y = int.from_bytes(pub[1:33], "big"), int.from_bytes(pub[33:], "big")
        if x >= P or y >= P:
            return None
        if pub[0] in (6, 7) and (y & 1) != (pub[0] & 1):
            return None
        return (x, y) if on_curve(x, y) else None
    return None


def reencode(pub: bytes):
    """gsv_pubkey_parse_batch: (65 bytes, ok)"""
    pt = parse_pubkey(pub)
    if pt is None:
        return bytes(65), 0
    return b"\x04" + be32(pt[0]) + be32(pt[1]), 1


def encode(pt, form):
    """form: 4 (uncompressed), 2 (compressed, the prefix takes y's parity), 6 (hybrid, likewise)"""
    x, y = pt
    if form == 4:
        return b"\x04" + be32(x) + be32(y)
    if form == 2:
        return bytes([2 | (y & 1)]) + be32(x)
    if form == 6:
        return bytes([6 | (y & 1)]) + be32(x) + be32(y)
    raise ValueError(form)


def verify(msg32: bytes, sig64: bytes, pub: bytes) -> bool:
    """rules 1-3 of gsv_ecdsa_verify_batch"""
    if len(msg32) != 32 or len(sig64) != 64:
        return False
    r, s = int.from_bytes(sig64[:32], "big"), int.from_bytes(sig64[32:], "big")
    if not (0 < r < N and 0 < s < N) or s > HALF_N:
        return False
    pt = parse_pubkey(pub)
    if pt is None:
        return False
    m = int.from_bytes(msg32, "big") % N
    si = pow(s, -1, N)
    X = M.ec_add(M.ec_mul(m * si % N, G), M.ec_mul(r * si % N, pt))
    if X is None:
        return False
    # the projective comparison of the device, affine here: x == r, or x == r + n when r < p - n
    return X[0] == r or (r < P - N and X[0] == r + N)


def craft_verify(Pt, u1, u2, u1G=False):
    """(msg32, sig64) whose verification under Pt computes u1 G + u2 Pt, or None when that signature
    would have s > n/2 or r = 0 (the caller draws another Pt: half the draws qualify).
    R = u1 G + u2 Pt, r = R_x mod n, s = r / u2, msg = u1 s.  u1G: u1 G when the caller has it."""
    assert u2 % N
    R = M.ec_add(M.ec_mul(u1, G) if u1G is False else u1G, M.ec_mul(u2, Pt))
    if R is None:
        return None
    r = R[0] % N
    if r == 0:
        return None
    s = r * pow(u2, -1, N) % N
    if s > HALF_N:
        return None
    return be32(u1 * s % N), be32(r) + be32(s)


def point_for(u1, u2, seed=1):
    """(Pt, msg32, sig64): the first curve point with x = seed, seed + 1, ... (mod p; its y parity is
    x's low bit) for which craft_verify gives a lower-s signature"""
    u1G = M.ec_mul(u1, G)
    x = seed % P
    while True:
        Pt = M.lift_x(x, x & 1)
        c = craft_verify(Pt, u1, u2, u1G) if Pt is not None else None
        if c is not None:
            return Pt, c[0], c[1]
        x = (x + 1) % P


def sign(d, msg32, k):
    """lower-s ECDSA with an explicit nonce: sig64"""
    R = M.ec_mul(k, G)
    r = R[0] % N
    s = pow(k, -1, N) * (int.from_bytes(msg32, "big") + r * d) % N
    assert r and s
    if s > HALF_N:
        s = N - s
    return be32(r) + be32(s)


def first_x_above_n():
    """The first x > n with x^3 + 7 a square, as the point with even y.  (x = n itself is an x
    coordinate of the curve, but r = x - n = 0 there, which rule 1 rejects: the r + n branch starts at
    the next one.)"""
    assert M.lift_x(N, 0) is not None
    x = N + 1
    while True:
        pt = M.lift_x(x, 0)
        if pt is not None:
            return pt
        x += 1


def rejection_cases(msg32, sig64, pt):
    """[(name, msg32, sig64, key bytes)]: each a single mutation of a valid item (msg32, sig64, pt) that
    rule 1, 2 or 3 rejects.  The names say which."""
    x, y = pt
    r, s = int.from_bytes(sig64[:32], "big"), int.from_bytes(sig64[32:], "big")
    key = encode(pt, 4)
    out = []

    def flip(b, bit):
        b = bytearray(b)
        b[bit // 8] ^= 1 << (bit % 8)
        return bytes(b)

    out.append(("msg bit", flip(msg32, 77), sig64, key))
    out.append(("r bit", msg32, flip(sig64, 13), key))
    out.append(("s bit", msg32, flip(sig64, 256 + 100), key))
    out.append(("key x bit", msg32, sig64, flip(key, 8 + 50)))
    out.append(("high s", msg32, be32(r) + be32(N - s), key))
    for v in (0, N, N + 1, (1 << 256) - 1):
        out.append(("r = %x" % v, msg32, be32(v) + be32(s), key))
        out.append(("s = %x" % v, msg32, be32(r) + be32(v), key))
    for name, k in key_rejections(pt):
        out.append((name, msg32, sig64, k))
    return out


def key_rejections(pt):
    """[(name, key bytes)]: encodings of (or near) the valid point pt that rule 2 rejects"""
    x, y = pt
    full, comp, hyb = encode(pt, 4), encode(pt, 2), encode(pt, 6)
    out = [("hybrid wrong parity", bytes([hyb[0] ^ 1]) + hyb[1:]),
           ("prefix 05", b"\x05" + full[1:]),
           ("prefix 00", b"\x00" + full[1:]),
           ("compressed prefix 00", b"\x00" + comp[1:]),
           ("65 bytes with prefix 02", bytes([comp[0]]) + full[1:]),
           ("33 bytes with prefix 04", b"\x04" + comp[1:]),
           ("x = p", b"\x04" + be32(P) + be32(y)),
           ("compressed x = p", b"\x02" + be32(P)),
           ("y = p", b"\x04" + be32(x) + be32(P)),
           ("x > p", b"\x04" + be32(P + 1) + be32(y)),
           ("compressed x > p", b"\x03" + be32((1 << 256) - 1)),
           ("off the curve", b"\x04" + be32(x) + be32((y + 1) % P)),
           ("hybrid off the curve", bytes([6 | ((y + 1) % P & 1)]) + be32(x) + be32((y + 1) % P))]
    xn = 1
    while M.lift_x(xn, 0) is not None:  # the first x whose x^3 + 7 is a non-residue
        xn += 1
    out.append(("compressed non-residue", b"\x02" + be32(xn)))
    for n in BAD_LENGTHS:
        out.append(("length %d" % n, (full + b"\x00")[:n] if n else b""))
    out.append(("length 32 compressed", comp[:32]))
    out.append(("length 34 compressed", comp + b"\x00"))
    return out


# ---------------------------------------------------------------- the bulk set and its expectation by recovery
def bulk_items(oracle, seed, n):
    """[(msg32, sig64, key bytes)]: even items valid (keys alternately compressed and uncompressed), odd
    items one mutation each"""
    rng = random.Random(seed)
    items = []
    for i in range(n):
        sk = be32(rng.randrange(1, N))
        msg = bytes(rng.getrandbits(8) for _ in range(32))
        sig = oracle.secp_sign(msg, sk, be32(rng.randrange(1, N)))[:64]
        pub = oracle.secp_pubkey(sk)
        pt = (int.from_bytes(pub[1:33], "big"), int.from_bytes(pub[33:], "big"))
        key = encode(pt, 2 if (i >> 1) & 1 else 4)
        if i & 1:
            kind = (i >> 2) % 8
            r, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
            if kind == 0:
                msg = bytes([msg[0] ^ 1]) + msg[1:]
            elif kind == 1:
                sig = be32(r ^ (1 << rng.randrange(255))) + sig[32:]
            elif kind == 2:
                sig = sig[:32] + be32(s ^ (1 << rng.randrange(250)))
            elif kind == 3:
                sig = sig[:32] + be32(N - s)
            elif kind == 4:  # another key that parses
                other = oracle.secp_pubkey(be32(rng.randrange(1, N)))
                key = other if len(key) == 65 else bytes([2 | (other[64] & 1)]) + other[1:33]
            elif kind == 5:  # the negated key: parses, same x
                key = encode((pt[0], P - pt[1]), 2 if len(key) == 33 else 4)
            elif kind == 6:
                key = key_rejections(pt)[rng.randrange(len(key_rejections(pt)))][1]
            else:
                sig = be32((0, N, r + N if r + N < 1 << 256 else N)[rng.randrange(3)]) + sig[32:]
        items.append((msg, sig, key))
    return items


def identity_expected(recover, msg, sig, key):
    """verify's verdict by recovery: recover(msg32, sig65) -> 65-byte key or None"""
    pub, ok = reencode(key)
    if not ok or int.from_bytes(sig[32:], "big") > HALF_N:
        return False
    return any(recover(msg, sig + bytes([recid])) == pub for recid in range(4))
