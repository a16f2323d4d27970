"""CPU tests of the secp256k1 recovery's scalar schedule (tests/secp_glv_model.py: the split, the
lattice-vector step, the odd-digit recoding and the ladder order of secp256k1_glv.cuh in Python integers)
and of the oracle's chain checker that the GPU sweep of the comb table relies on.  No GPU.

The bounds asserted here are the ones secp256k1_glv.cuh states in comments and relies on: both GLV halves
odd and below 2^130 (GLV_DIGITS windows of GLV_W bits), every digit odd within the 2^(GLV_W-1)-entry
table, the top digit included (recode_glv takes it unsigned: above 2^GLV_W - 1 it would run into the
sign bit of the digit code)."""
import random

import numpy as np
import pytest

import secp_glv_model as M

N, LAM = M.N, M.LAMBDA


# ---------------------------------------------------------------- the source parse
def test_parse_reads_the_headers_and_fails_loudly():
    assert (M.GLV_NT, M.GLV_DIGITS) == (1 << (M.GLV_W - 1), (130 + M.GLV_W - 1) // M.GLV_W)
    assert M.COMB_WINDOWS == (256 + M.COMB_BITS - 1) // M.COMB_BITS
    assert N == 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141  # SEC 2, the group order
    assert M.P == 2 ** 256 - 2 ** 32 - 977 and M.HALF_N == N // 2
    assert M.lift_x(M.GX, M.GY & 1) == M.G
    txt = "constexpr int GLV_W = 5;\n__device__ constexpr uint32_t K[8] = {1u, 0x2u, 0u, 0u, 0u, 0u, 0u, 0x80000000u};"
    assert M.parse_int("GLV_W", text=txt) == 5
    assert M.parse_words("K", text=txt) == 1 + (2 << 32) + (0x80000000 << 224)
    for bad in ("constexpr int GLV_W = foo();", "constexpr int GLV_W = OTHER + 1;", "",
                "constexpr int GLV_W = 4;\nconstexpr int GLV_W = 5;"):
        with pytest.raises(ValueError):
            M.parse_int("GLV_W", text=bad)
    for bad in ("", "constexpr uint32_t K[8] = {1u, 2u};", "constexpr uint32_t K[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};",
                "constexpr uint32_t K[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0x100000000u};",
                "constexpr uint32_t K[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, X};"):
        with pytest.raises(ValueError):
            M.parse_words("K", text=bad)


def test_lattice_constants():
    assert pow(LAM, 3, N) == 1 and LAM != 1
    assert pow(M.BETA, 3, M.P) == 1 and M.BETA != 1
    assert M.ec_mul(LAM, M.G) == (M.BETA * M.GX % M.P, M.GY)  # lambda (x, y) = (beta x, y)
    for name, (a, b) in M.BRANCH_VECTORS.items():
        assert (a + b * LAM) % N == 0, name
    # parities glv_make_odd's table relies on: v1 odd/odd, v2 even/odd, v3 = v1 + v2 odd/even (as signed values)
    par = {k: (abs(M.signed(a)) & 1, abs(M.signed(b)) & 1) for k, (a, b) in M.BRANCH_VECTORS.items()}
    assert par == {"v1": (1, 1), "v2": (0, 1), "v3": (1, 0), "none": (0, 0)}
    assert (M.GLV_V3A, M.GLV_V3B) == ((M.GLV_V1A + M.GLV_V2A) % N, (M.GLV_V1B + M.GLV_V1A) % N)
    assert all(abs(M.signed(v)).bit_length() <= 129 for v in M.GLV_V.values())
    # the split's constants: -b1, -b2 and g1, g2 = round(2^272 b2 / n), round(2^272 (-b1) / n)
    # (libsecp256k1 scalar_impl.h), with (a1, b1) = v1 and (a2, b2) = (v2a, a1)
    b1, b2 = M.signed(M.GLV_V1B), M.signed(M.GLV_V1A)
    assert (M.MINUS_B1, M.MINUS_B2) == (-b1 % N, -b2 % N)
    assert M.GLV_G1 == ((b2 << 272) + N // 2) // N and M.GLV_G2 == ((-b1 << 272) + N // 2) // N


# ---------------------------------------------------------------- the three families, one pass each
_DEC = {c: M.decode(c) for c in range(1 << M.GLV_W)}
assert all(d & 1 and abs(d) < 1 << M.GLV_W for d in _DEC.values())


class _Props:
    """the schedule's properties, asserted for every scalar it is shown; keeps the widest magnitude"""

    def __init__(self):
        self.bits = 0
        self.count = 0

    def __call__(self, s):
        u, lim = s.u2, (1 << M.GLV_W) - 1
        r1, r2 = s.split
        assert (r1 + r2 * LAM) % N == u, hex(u)
        assert max(abs(M.signed(r1)), abs(M.signed(r2))) < 1 << 128, hex(u)  # the split's own bound
        k1, k2 = s.k
        assert (k1 + k2 * LAM) % N == u, hex(u)
        for neg, mag, skew, codes, digits, rest, k in ((s.neg1, s.mag1, s.skew1, s.codes1, s.digits1, s.rest1, k1),
                                                       (s.neg2, s.mag2, s.skew2, s.codes2, s.digits2, s.rest2, k2)):
            assert (N - mag if neg else mag) % N == k
            assert mag & 1 and mag < 1 << 130 and skew == 0, (hex(u), hex(mag))
            assert rest == 0 and len(digits) == M.GLV_DIGITS
            assert -lim <= min(digits) and max(digits) <= lim, (hex(u), digits)
            # as the ladder reads the codes: odd digits of the table, the (unsigned) top digit included
            assert [_DEC.get(c) for c in codes] == digits, (hex(u), digits)
            assert sum(d << (M.GLV_W * i) for i, d in enumerate(digits)) == mag
            self.bits = max(self.bits, mag.bit_length())
        self.count += 1


def test_random_scalars():
    rng = random.Random(20260131)
    props = _Props()
    events, wrong, branches = M.walk((rng.randrange(1, N) for _ in range(100_000)), props)
    assert props.count == 100_000 and props.bits <= 130
    assert not wrong and not events, ([hex(u) for u in wrong[:4]], {hex(u): e for u, e in events.items()})
    assert all(branches[b] >= 20_000 for b in M.BRANCH_VECTORS), branches


@pytest.fixture(scope="module")
def small():
    props = _Props()
    res = M.walk_family("small", props)
    assert props.count == 301 * 301 - 1 and props.bits <= 130
    return res


def test_small_family_branches_and_split(small):
    events, wrong, branches = small
    assert not wrong, [hex(u) for u in wrong[:4]]
    assert all(branches[b] >= (301 * 301 - 1) // 5 for b in M.BRANCH_VECTORS), branches
    # tiny splits: the halves are exactly (a, b), so the lattice vector alone decides the magnitudes
    for u, a, b in M.small_family(150)[::97]:
        assert tuple(M.signed(k) for k in M.split_lambda(u)) == (a, b)


def test_small_family_ladder_exceptions(small):
    events = small[0]
    assert all(kind in ("dbl", "inf", "identity") for ev in events.values() for kind, _, _ in ev)
    assert any(kind == "dbl" for ev in events.values() for kind, _, _ in ev)
    assert ("dbl", 0, 1) in events[(-26 * LAM) % N]
    assert M.split_lambda((-26 * LAM) % N) == (0, N - 26) and M.Schedule((-26 * LAM) % N).branch == "v1"
    # whatever the ladder meets, infinities included, is in the set the GPU tests run
    assert set(events) <= set(M.exceptional_scalars())


def test_near_constant_family():
    fam = M.family("near")
    assert len(fam) > 18_000 and len(set(fam)) == len(fam) and 0 not in fam
    assert len(M.near_constant_centres()) == 6 + 10 + sum(m - 1 for m in (3, 5, 7, 9, 11, 13, 128))
    props = _Props()
    events, wrong, branches = M.walk_family("near", props)
    assert props.count == len(fam) and props.bits <= 130 and not wrong
    assert set(events) <= set(M.exceptional_scalars())


def test_comb_digits():
    rng = random.Random(5)
    for u in [0, 1, N - 1, (1 << 256) - 1] + [rng.randrange(N) for _ in range(200)]:
        d = M.comb_digits(u)
        assert len(d) == M.COMB_WINDOWS and sum(v << (M.COMB_BITS * w) for w, v in enumerate(d)) == u
    # u1 < n keeps the top window's digit at or below this; entries above it are unreachable
    assert M.comb_digits(N - 1)[-1] == (N - 1) >> (M.COMB_BITS * (M.COMB_WINDOWS - 1))


def test_crafted_signature_recovers_chosen_scalars(oracle):
    """sig = (x_R, u2 x_R, parity of y_R), msg = -u1 x_R recovers u1 G + u2 R: oracle vs Python integers"""
    rng = random.Random(12)
    for u1, u2 in [(rng.randrange(N), rng.randrange(1, N)), (0, (-26 * LAM) % N), (1, 1), (N - 1, N - 1),
                   (1 << M.COMB_BITS, 3)]:
        x = rng.randrange(1, N)
        while M.lift_x(x, 0) is None:
            x += 1
        R = M.lift_x(x, rng.randrange(2))
        msg, r, s, recid = M.craft(R, u1, u2)
        rc, pub = oracle.ecrecover(msg.to_bytes(32, "big"), r.to_bytes(32, "big") + s.to_bytes(32, "big") + bytes([recid]))
        q = M.recover_expected(R, u1, u2)
        assert rc == 1 and pub == b"\x04" + q[0].to_bytes(32, "big") + q[1].to_bytes(32, "big")


# ---------------------------------------------------------------- the oracle's chain checker
def _rows(points):
    return np.frombuffer(b"".join(x.to_bytes(32, "big") + y.to_bytes(32, "big") for x, y in points),
                         np.uint8).reshape(-1, 64).copy()


def test_chain_check(oracle):
    rng = random.Random(3)
    base = M.ec_mul(1 << 40, M.G)
    b64 = bytes(_rows([base])[0])
    start = M.ec_mul(rng.randrange(1, N), M.G)
    chain = [start]
    for _ in range(299):
        chain.append(M.ec_add(chain[-1], base))
    good = _rows(chain)
    for threads in (1, 3, 8, 64):
        assert oracle.secp_chain_check(good, b64, threads) == oracle.CHAIN_OK
    assert oracle.secp_chain_check(good[:1], b64) == oracle.CHAIN_OK
    assert oracle.secp_chain_check(good[:2], b64, 8) == oracle.CHAIN_OK
    # one coordinate of one point altered: x or y, any byte, first, inner, thread-boundary and last rows
    for i in (0, 1, 37, 38, 74, 75, 150, 298, 299):
        for col in (0, 17, 31, 32, 50, 63):
            bad = good.copy()
            bad[i, col] ^= 1 << rng.randrange(8)
            for threads in (1, 8):
                assert oracle.secp_chain_check(bad, b64, threads) == i, (i, col, threads)
    # a point replaced by another curve point (its negative; a multiple of the base off by one)
    for i in (1, 75, 299):
        bad = good.copy()
        bad[i] = _rows([(chain[i][0], M.P - chain[i][1])])[0]
        assert oracle.secp_chain_check(bad, b64) == i
        bad[i] = _rows([M.ec_add(chain[i], base)])[0]
        assert oracle.secp_chain_check(bad, b64) == i
    # two points swapped, neighbours and distant ones: the lower row is the first that is not its
    # predecessor + B (row 1 when row 0 is one of the two)
    for i, j in ((1, 2), (5, 200), (74, 75), (298, 299), (0, 1), (0, 150)):
        bad = good.copy()
        bad[[i, j]] = bad[[j, i]]
        for threads in (1, 8):
            assert oracle.secp_chain_check(bad, b64, threads) == max(i, 1), (i, j, threads)
    # a coordinate at or above p is refused even where its residue is the right one; so is x = y = 0
    one = M.lift_x(1, 0)
    assert one is not None
    low = [M.ec_add(one, M.ec_mul(N - 3 << 40, M.G))]
    for _ in range(6):
        low.append(M.ec_add(low[-1], base))
    assert low[3] == one
    rows = _rows(low)
    assert oracle.secp_chain_check(rows, b64) == oracle.CHAIN_OK
    rows[3, :32] = np.frombuffer((1 + M.P).to_bytes(32, "big"), np.uint8)
    assert oracle.secp_chain_check(rows, b64) == 3
    bad = good.copy()
    bad[4] = 0
    assert oracle.secp_chain_check(bad, b64) == 4
    # the degenerate step (a row with the base's own x) has a code of its own, as has a bad base
    deg = _rows([M.ec_mul(k << 40, M.G) for k in range(1, 6)])
    assert oracle.secp_chain_check(deg, b64) == oracle.CHAIN_DEGENERATE
    assert oracle.secp_chain_check(deg[1:], b64) == oracle.CHAIN_OK
    assert oracle.secp_chain_check(good, bytes(64)) == oracle.CHAIN_BAD_BASE
