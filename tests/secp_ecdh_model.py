"""secp256k1 ScalarMult, the ECDH shared secret and the ECIES key derivation in Python integers: the
semantics gsv_secp256k1_scalar_mul_batch and gsv_ecdh_batch pin (include/gsv.h), restated from the
reference's cgo path (crypto/secp256k1/ext.h secp256k1_ext_scalar_mul, crypto/ecies/ecies.go
GenerateShared, concatKDF and the keys Encrypt derives).  Self-contained: plain affine arithmetic, the
constants written out, hashlib for SHA-256.

Also the edge cases the fixture (tests/golden/make_secp_ecdh.py) and the GPU tests share.
"""
import hashlib
import random

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
GX = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
GY = 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8
G = (GX, GY)
# the endomorphism (x, y) -> (BETA x, y) is multiplication by LAMBDA
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE

ST_OK, ST_INVALID_KEY, ST_INVALID_CURVE = 0, 11, 12

# the reference's own static vector (crypto/ecies/ecies_test.go:458-485 TestSharedKeyStatic)
STATIC_PRV1 = bytes.fromhex("7ebbc6a8358bc76dd73ebc557056702c8cfc34e5cfcd90eb83af0347575fd2ad")
STATIC_PRV2 = bytes.fromhex("6a3d6396903245bba5837752b9e0348874e72db0c4e11e9c485a81b4ea4353b9")
STATIC_SHARED = bytes.fromhex("167ccc13ac5e8a26b131c3446030c60fbfac6aa8e31149d0869f93626a4cdf62")


def be32(x):
    return int(x).to_bytes(32, "big")


def on_curve(x, y):
    return (y * y - x * x * x - 7) % P == 0


def ec_add(a, b):
    """a + b on y^2 = x^3 + 7 over F_p; None is the identity"""
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
    return x, (l * (a[0] - x) - a[1]) % P


def ec_mul(k, pt):
    acc = None
    while k:
        if k & 1:
            acc = ec_add(acc, pt)
        pt = ec_add(pt, pt)
        k >>= 1
    return acc


def ec_neg(pt):
    return pt[0], (P - pt[1]) % P


def lift_x(x, odd):
    """the curve point with this x and y of the given parity, or None"""
    c = (x * x * x + 7) % P
    y = pow(c, (P + 1) // 4, P)
    if y * y % P != c:
        return None
    return x, y if (y & 1) == odd else P - y


def cube_root(a):
    """a cube root of a mod p, or None (p = 7 mod 9: a^((p + 2) / 9) when a is a cube)"""
    assert P % 9 == 7
    r = pow(a, (P + 2) // 9, P)
    return r if pow(r, 3, P) == a % P else None


def pt64(pt):
    return be32(pt[0]) + be32(pt[1])


# ---------------------------------------------------------------- the rules
def scalar_mul(point64: bytes, scalar32: bytes):
    """gsv_secp256k1_scalar_mul_batch for one item: (status, out64)"""
    assert len(point64) == 64 and len(scalar32) == 32
    k = int.from_bytes(scalar32, "big")
    if k == 0 or k >= N:  # the reference's only failure, tested first
        return ST_INVALID_KEY, bytes(64)
    # fe_set_b32 with its verdict ignored: a coordinate >= p is reduced
    x = int.from_bytes(point64[:32], "big") % P
    y = int.from_bytes(point64[32:], "big") % P
    if not on_curve(x, y):  # the divergence: the reference multiplies on another curve
        return ST_INVALID_CURVE, bytes(64)
    R = ec_mul(k, (x, y))
    assert R is not None  # k in [1, n) and a point of order n (the curve's cofactor is 1)
    return ST_OK, pt64(R)


def kdf_keys(shared32: bytes) -> bytes:
    """Ke || Km of ECIES_AES128_SHA256 with s1 empty: K = SHA256(00 00 00 01 || X) (concatKDF with
    kdLen = 32: one hash), Ke = K[:16], Km = SHA256(K[16:])"""
    K = hashlib.sha256(b"\x00\x00\x00\x01" + shared32).digest()
    return K[:16] + hashlib.sha256(K[16:]).digest()


def ecdh(pub64: bytes, seckey32: bytes):
    """gsv_ecdh_batch for one item: (status, shared32, keys48)"""
    st, out = scalar_mul(pub64, seckey32)
    if st != ST_OK:
        return st, bytes(32), bytes(48)
    return st, out[:32], kdf_keys(out[:32])


def generate_shared(prv: bytes, pub64: bytes, sk_len: int, mac_len: int) -> bytes:
    """ecies.GenerateShared for skLen + macLen = 32 (ecies.go:134-137: x.Bytes() right-aligned)"""
    assert sk_len + mac_len == 32
    st, out = scalar_mul(pub64, prv.rjust(32, b"\0"))
    assert st == ST_OK
    xb = int.from_bytes(out[:32], "big").to_bytes(32, "big").lstrip(b"\0")
    return bytes(32 - len(xb)) + xb


# ---------------------------------------------------------------- the shared cases
BAD_SCALARS = (0, N, N + 1, 2**256 - 1)
GOOD_EDGE_SCALARS = (1, N - 1)
OFF_CURVE_POINTS = ((GX, GY + 1), (0, 0), (GX, P - 1))
# the ladder's edges: the four parity cases of glv_make_odd, zero GLV halves, the top-digit start
LADDER_SCALARS = (1, 2, 3, N - 1, N - 2, (N - 1) // 2, (N + 1) // 2, LAMBDA, N - LAMBDA, LAMBDA - 1, LAMBDA + 1,
                  2 * LAMBDA % N, 1 + LAMBDA, 2 + 2 * LAMBDA, LAMBDA * LAMBDA % N, 2**127, 2**128 - 1, 2**128,
                  2**128 + 1, 2**255)
SEED = 121


def point_x1():
    """the point with x = 1 and even y"""
    return lift_x(1, 0)


def random_point(rng):
    return ec_mul(rng.randrange(1, N), G)


def ladder_points():
    """G, -G, 2G, lambda G = (beta Gx, Gy), the point with x = 1, a seeded random point"""
    lam_g = (BETA * GX % P, GY)
    assert lam_g == ec_mul(LAMBDA, G)
    return [G, ec_neg(G), ec_mul(2, G), lam_g, point_x1(), random_point(random.Random(SEED + 1))]


def small_y_point(limit=1 << 16):
    """a curve point with the smallest y in [1, limit) (so that y + p fits 32 bytes), or None"""
    for y in range(1, limit):
        x = cube_root((y * y - 7) % P)
        if x is not None:
            assert on_curve(x, y)
            return x, y
    return None


def unreduced_cases():
    """[(tag, point64 written with a coordinate >= p, the same point reduced)]: coordinates below
    2^32 + 977 are the only ones with a second 32-byte form"""
    out = []
    t = point_x1()
    out.append(("x+p", be32(t[0] + P) + be32(t[1]), pt64(t)))
    s = small_y_point()
    if s is not None:
        out.append(("y+p", be32(s[0]) + be32(s[1] + P), pt64(s)))
    return out


def leading_zero_case(rng):
    """(point64, scalar32) whose product is the point with x = 1: P = k^-1 T"""
    k = rng.randrange(1, N)
    return pt64(ec_mul(pow(k, -1, N), point_x1())), be32(k)


def edge_rows():
    """[(tag, point64, scalar32)]: the scalar and curve rules, the ladder's edges on G and three of them on
    every other ladder point, coordinates >= p with their reduced twins, the leading-zero X, and the
    static vector both ways"""
    rng = random.Random(SEED)
    rows = []
    g64 = pt64(G)
    for k in BAD_SCALARS:
        rows.append(("bad scalar", g64, be32(k)))
    for k in GOOD_EDGE_SCALARS:
        rows.append(("edge scalar", g64, be32(k)))
    for pt in OFF_CURVE_POINTS:
        rows.append(("off curve", be32(pt[0]) + be32(pt[1]), be32(rng.randrange(1, N))))
    rows.append(("bad scalar, off curve", be32(GX) + be32(GY + 1), be32(0)))
    rows.append(("bad scalar, off curve", be32(0) + be32(0), be32(N)))
    for k in LADDER_SCALARS:
        rows.append(("ladder", g64, be32(k)))
    for pt in ladder_points()[1:]:
        for k in (LAMBDA, (N + 1) // 2, 2**128):
            rows.append(("ladder", pt64(pt), be32(k)))
    k = be32(rng.randrange(1, N))
    for tag, raw, red in unreduced_cases():
        rows.append((tag, raw, k))
        rows.append((tag + " reduced", red, k))
    rows.append(("leading zeros",) + leading_zero_case(rng))
    pub1 = pt64(ec_mul(int.from_bytes(STATIC_PRV1, "big"), G))
    pub2 = pt64(ec_mul(int.from_bytes(STATIC_PRV2, "big"), G))
    rows.append(("static a(bG)", pub2, STATIC_PRV1))
    rows.append(("static b(aG)", pub1, STATIC_PRV2))
    return rows


def random_rows(count, seed=SEED + 2):
    rng = random.Random(seed)
    return [("random", pt64(random_point(rng)), be32(rng.randrange(1, N))) for _ in range(count)]
