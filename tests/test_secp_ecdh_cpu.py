"""CPU tests of the ScalarMult / ECDH feature: the boundary (header, exports, bindings, argument checks
that precede every HIP call, the new status code, the Python mirrors' host-side rules) and the recorded
results of the reference's secp256k1_ext_scalar_mul (tests/golden/secp_ecdh.json) against the
pure-Python model (tests/secp_ecdh_model.py).  No GPU."""
import ctypes
import hashlib
import os
import re

import pytest

import secp_ecdh_model as M
from conftest import ROOT, golden

NEW = ["gsv_secp256k1_scalar_mul_batch", "gsv_secp256k1_scalar_mul_batch_dev", "gsv_ecdh_batch", "gsv_ecdh_batch_dev"]


@pytest.fixture(scope="module")
def fx():
    return golden("secp_ecdh.json")


def test_boundary_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, "include", "gsv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from gsv import _lib
    L = _lib.load()
    bound = {n: a for n, _, a in _lib.SIGNATURES}
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, code), s
        assert hasattr(L, s), s
        assert s in bound, s
        # the binding's arity is the header's
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % s, code).group(1)
        assert len(bound[s]) == decl.count(",") + 1, s
    assert int(re.search(r"#define GSV_ST_INVALID_CURVE (\d+)", txt).group(1)) == _lib.ST_INVALID_CURVE == 12
    assert int(re.search(r"#define GSV_ST_INVALID_KEY (\d+)", txt).group(1)) == _lib.ST_INVALID_KEY == 11
    assert int(re.search(r"#define GSV_ABI_VERSION (\d+)", txt).group(1)) == 2
    assert _lib.STATUS_STRINGS[_lib.ST_INVALID_CURVE] == "ecies: invalid elliptic curve"
    assert M.ST_INVALID_KEY == _lib.ST_INVALID_KEY and M.ST_INVALID_CURVE == _lib.ST_INVALID_CURVE


def test_null_arguments_are_refused_without_a_device():
    """argument checks precede every HIP call: a NULL context, and (with a context that is never
    dereferenced) a NULL required pointer, both ECDH outputs NULL, n past 2^32 - 1"""
    from gsv import _lib
    L = _lib.load()
    E = _lib.E_INVALID_ARG
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.gsv_secp256k1_scalar_mul_batch(None, p, p, 1, p, p) == E
    assert L.gsv_secp256k1_scalar_mul_batch_dev(None, p, p, 1, p, p, None) == E
    assert L.gsv_ecdh_batch(None, p, p, 1, p, p, p) == E
    assert L.gsv_ecdh_batch_dev(None, p, p, 1, p, p, p, None) == E
    fake = p  # a non-NULL context: the argument checks return before it is read
    for k in range(4):
        a = [p, p, p, p]
        a[k] = None
        assert L.gsv_secp256k1_scalar_mul_batch(fake, a[0], a[1], 1, a[2], a[3]) == E
        assert L.gsv_secp256k1_scalar_mul_batch_dev(fake, a[0], a[1], 1, a[2], a[3], None) == E
    for a in ([None, p, p, p, p], [p, None, p, p, p], [p, p, p, p, None], [p, p, None, None, p]):
        assert L.gsv_ecdh_batch(fake, a[0], a[1], 1, a[2], a[3], a[4]) == E
        assert L.gsv_ecdh_batch_dev(fake, a[0], a[1], 1, a[2], a[3], a[4], None) == E
    big = 1 << 32
    assert L.gsv_secp256k1_scalar_mul_batch(fake, p, p, big, p, p) == E
    assert L.gsv_ecdh_batch_dev(fake, p, p, big, p, p, p, None) == E
    # n = 0 is success and touches nothing (host forms: before any HIP call)
    assert L.gsv_secp256k1_scalar_mul_batch(fake, None, None, 0, None, None) == 0
    assert L.gsv_ecdh_batch(fake, None, None, 0, None, None, None) == 0


def test_python_mirrors_host_side_rules():
    """what the mirrors decide before any GPU call"""
    from gsv import crypto, ecies
    with pytest.raises(ValueError):
        crypto.ScalarMult(M.GX, M.GY, bytes(33))  # the Go panic
    with pytest.raises(ecies.ErrSharedKeyTooBig):
        ecies.GenerateShared(1, M.pt64(M.G), 32, 32)
    with pytest.raises(ecies.ErrSharedKeyTooBig):
        ecies.GenerateShared(1, M.pt64(M.G), 16, 17)
    with pytest.raises(ValueError):
        ecies.GenerateShared(1, M.pt64(M.G), 8, 8)  # X may be longer: the reference would panic
    with pytest.raises(ValueError):
        ecies.GenerateShared(1, bytes(63), 16, 16)
    assert issubclass(ecies.ErrInvalidCurve, ValueError)
    assert ecies.ErrSharedKeyIsPointAtInfinity.__doc__ == "ecies: shared key is point at infinity"
    assert (crypto.S256_GX, crypto.S256_GY) == M.G


def test_model_constants():
    assert M.on_curve(*M.G) and M.ec_mul(M.N, M.G) is None
    assert pow(M.BETA, 3, M.P) == 1 and M.BETA != 1 and pow(M.LAMBDA, 3, M.N) == 1 and M.LAMBDA != 1
    assert M.ec_mul(M.LAMBDA, M.G) == (M.BETA * M.GX % M.P, M.GY)
    assert len(M.LADDER_SCALARS) == 20 and all(0 < k < M.N for k in M.LADDER_SCALARS)
    assert all(M.on_curve(*pt) for pt in M.ladder_points()) and len(M.ladder_points()) == 6
    assert not any(M.on_curve(*pt) for pt in M.OFF_CURVE_POINTS)


def test_fixture_shape(fx):
    rows = fx["rows"]
    assert len(rows) == 96
    tags = [r["tag"] for r in rows]
    edge = M.edge_rows()
    assert tags[:len(edge)] == [t for t, _, _ in edge] and set(tags[len(edge):]) == {"random"}
    for (t, pt, k), r in zip(edge, rows):  # the fixture is the model's case list
        assert r["point"] == pt.hex() and r["scalar"] == k.hex(), t
    assert fx["unreduced"] == [t for t, _, _ in M.unreduced_cases()]
    assert "x+p" in fx["unreduced"]
    st = [r["status"] for r in rows]
    assert st.count(11) == 6 and st.count(12) == 3 and st.count(0) == 87


def test_model_equals_the_reference_on_every_row(fx):
    for r in fx["rows"]:
        pt, k = bytes.fromhex(r["point"]), bytes.fromhex(r["scalar"])
        st, out = M.scalar_mul(pt, k)
        assert st == r["status"], r["tag"]
        assert out.hex() == r["out"], r["tag"]
        # status 11 exactly where the reference fails, and there it leaves its buffer alone
        assert (st == M.ST_INVALID_KEY) == (r["ref_rc"] == 0), r["tag"]
        if r["ref_rc"] == 0:
            assert r["ref_out"] == r["point"]
        if st == M.ST_OK:
            assert r["out"] == r["ref_out"], r["tag"]
        else:
            assert r["out"] == bytes(64).hex() and r["shared"] == bytes(32).hex() and r["keys48"] == bytes(48).hex()
        if st == M.ST_INVALID_CURVE:  # the divergence, pinned: the reference returns 1 and an artefact
            assert r["ref_rc"] == 1, r["tag"]  # (for (0, 0) the artefact is itself (0, 0))
        st2, shared, keys = M.ecdh(pt, k)
        assert (st2, shared.hex(), keys.hex()) == (st, r["shared"], r["keys48"]), r["tag"]


def test_kdf_is_the_reference_construction(fx):
    """keys48 restated from ecies.go with hashlib alone: concatKDF's loop for kdLen = 32, then Km"""
    for r in fx["rows"]:
        if r["status"] != 0:
            continue
        z = bytes.fromhex(r["shared"])
        reps = ((32 + 7) * 8) // (64 * 8)
        k, counter = b"", 1
        for _ in range(reps + 1):
            k += hashlib.sha256(counter.to_bytes(4, "big") + z + b"").digest()
            counter += 1
        k = k[:32]
        assert (k[:16] + hashlib.sha256(k[16:]).digest()).hex() == r["keys48"]


def test_unreduced_coordinates_give_the_reduced_points_result(fx):
    rows = {r["tag"]: r for r in fx["rows"]}
    for t in fx["unreduced"]:
        a, b = rows[t], rows[t + " reduced"]
        assert a["point"] != b["point"] and a["scalar"] == b["scalar"]
        assert a["ref_rc"] == b["ref_rc"] == 1 and a["ref_out"] == b["ref_out"] and a["status"] == b["status"] == 0


def test_leading_zero_row(fx):
    r = [r for r in fx["rows"] if r["tag"] == "leading zeros"][0]
    assert r["shared"] == (bytes(31) + b"\x01").hex() and r["ref_rc"] == 1
    assert M.generate_shared(bytes.fromhex(r["scalar"]), bytes.fromhex(r["point"]), 16, 16) == bytes(31) + b"\x01"


def test_static_vector_both_ways(fx):
    s = fx["static"]
    a, b = bytes.fromhex(s["prv1"]), bytes.fromhex(s["prv2"])
    assert (a, b, bytes.fromhex(s["shared"])) == (M.STATIC_PRV1, M.STATIC_PRV2, M.STATIC_SHARED)
    pub_a = M.pt64(M.ec_mul(int.from_bytes(a, "big"), M.G))
    pub_b = M.pt64(M.ec_mul(int.from_bytes(b, "big"), M.G))
    assert M.generate_shared(a, pub_b, 16, 16) == M.STATIC_SHARED  # a (bG)
    assert M.generate_shared(b, pub_a, 16, 16) == M.STATIC_SHARED  # b (aG)
    rows = {r["tag"]: r for r in fx["rows"]}
    assert rows["static a(bG)"]["ref_out"][:64] == rows["static b(aG)"]["ref_out"][:64] == s["shared"]
    assert rows["static a(bG)"]["point"] == pub_b.hex() and rows["static b(aG)"]["point"] == pub_a.hex()
