"""GPU parity of batched ScalarMult and ECDH (k_ecdh) with the reference's own function:
oracle.ref().secp256k1_ext_scalar_mul (crypto/secp256k1/ext.h:104-142), called through ctypes on the
reference build, and the recorded rows of tests/golden/secp_ecdh.json.  Every comparison is byte for
byte over every item.  The derived keys are compared with hashlib's.  The one divergence (a point off
the curve is refused with ST_INVALID_CURVE) is checked against the fixture, which records what the
reference returns there."""
import ctypes
import random

import numpy as np
import pytest

import secp_ecdh_model as M
from conftest import golden

pytestmark = pytest.mark.gpu
N, P = M.N, M.P
SHAPES = [1, 63, 64, 65, 255, 256, 257]
GUARD = 0xEE
be32 = M.be32


def u8(b, width):
    return np.frombuffer(bytes(b), np.uint8).reshape(-1, width).copy()


@pytest.fixture(scope="module")
def R(oracle):
    r = oracle.ref()
    assert r is not None, "the reference build oracle/_ref is needed (built by __graft_entry__.build())"
    return r


def ref_mul(R, point64, scalar32):
    """(rc, the 64-byte buffer afterwards) of the reference's secp256k1_ext_scalar_mul"""
    buf = ctypes.create_string_buffer(bytes(point64), 64)
    rc = R.secp256k1_ext_scalar_mul(None, buf, ctypes.c_char_p(bytes(scalar32)))
    return int(rc), buf.raw


def keys48_of(shared):
    """hashlib's Ke || Km for every row of shared (n,32)"""
    return u8(b"".join(M.kdf_keys(bytes(x)) for x in shared), 48)


@pytest.fixture(scope="module")
def bulk(R):
    """4,096 seeded (point, scalar) with the reference's products, computed once; the points are the
    reference's own multiples of G"""
    rng = random.Random(0xECD4)
    g64 = M.pt64(M.G)
    pts, ks, outs = [], [], []
    for _ in range(4096):
        rc, pt = ref_mul(R, g64, be32(rng.randrange(1, N)))
        assert rc == 1
        k = be32(rng.randrange(1, N))
        rc, out = ref_mul(R, pt, k)
        assert rc == 1
        pts.append(pt)
        ks.append(k)
        outs.append(out)
    pts, ks, outs = u8(b"".join(pts), 64), u8(b"".join(ks), 32), u8(b"".join(outs), 64)
    keys = keys48_of(outs[:, :32])
    for a in (pts, ks, outs, keys):
        a.setflags(write=False)
    return pts, ks, outs, keys


def dev_run(ctx, pts, ks, want_shared=True, want_keys=True, stream=None):
    """the two _dev forms on one explicit stream, outputs over-allocated by a guard row:
    (out64, st, shared32, keys48, est) with n + 1 rows each; an output not asked for stays all guard"""
    import torch
    dev = torch.device("cuda", ctx.device)
    n = pts.shape[0]
    d_pt = torch.from_numpy(np.array(pts)).to(dev)
    d_k = torch.from_numpy(np.array(ks)).to(dev)
    outs = [torch.full(shape, GUARD, dtype=torch.uint8, device=dev)
            for shape in ((n + 1, 64), (n + 1,), (n + 1, 32), (n + 1, 48), (n + 1,))]
    d_out, d_st, d_sh, d_keys, d_est = outs
    torch.cuda.synchronize()
    cs = stream or torch.cuda.Stream()
    ctx.secp256k1_scalar_mul_batch_dev(d_pt, d_k, d_out, d_st, stream=cs)
    ctx.ecdh_batch_dev(d_pt, d_k, d_sh if want_shared else None, d_keys if want_keys else None, d_est, stream=cs)
    cs.synchronize()
    return [o.cpu().numpy() for o in outs]


# ---------------------------------------------------------------- 1. recorded rows
def test_golden_rows_host_dev_and_mirrors(ctx):
    from gsv import _lib, crypto, ecies
    fx = golden("secp_ecdh.json")
    rows = fx["rows"]
    n = len(rows)
    pts = u8(b"".join(bytes.fromhex(r["point"]) for r in rows), 64)
    ks = u8(b"".join(bytes.fromhex(r["scalar"]) for r in rows), 32)
    want_out = u8(b"".join(bytes.fromhex(r["out"]) for r in rows), 64)
    want_sh = u8(b"".join(bytes.fromhex(r["shared"]) for r in rows), 32)
    want_keys = u8(b"".join(bytes.fromhex(r["keys48"]) for r in rows), 48)
    want_st = np.array([r["status"] for r in rows], np.uint8)
    # host forms, the three output modes
    out, st = ctx.secp256k1_scalar_mul_batch(pts, ks)
    assert (st == want_st).all(), np.nonzero(st != want_st)[0]
    assert (out == want_out).all(), np.nonzero((out != want_out).any(axis=1))[0]
    sh, none, st = ctx.ecdh_batch(pts, ks, want_shared=True, want_keys=False)
    assert none is None and (st == want_st).all() and (sh == want_sh).all()
    none, k48, st = ctx.ecdh_batch(pts, ks, want_shared=False, want_keys=True)
    assert none is None and (st == want_st).all() and (k48 == want_keys).all()
    sh, k48, st = ctx.ecdh_batch(pts, ks, want_shared=True, want_keys=True)
    assert (st == want_st).all() and (sh == want_sh).all() and (k48 == want_keys).all()
    # _dev forms
    for ws, wk in ((True, True), (True, False), (False, True)):
        d_out, d_st, d_sh, d_keys, d_est = dev_run(ctx, pts, ks, ws, wk)
        assert (d_out[:n] == want_out).all() and (d_st[:n] == want_st).all() and (d_est[:n] == want_st).all()
        assert (d_sh[:n] == want_sh).all() if ws else (d_sh == GUARD).all()
        assert (d_keys[:n] == want_keys).all() if wk else (d_keys == GUARD).all()
    # the Python mirrors
    o2, s2 = crypto.ScalarMultBatch(pts, ks, ctx)
    assert (o2 == want_out).all() and (s2 == want_st).all()
    s3, t3 = ecies.GenerateSharedBatch(ks, pts, ctx)
    assert (s3 == want_sh).all() and (t3 == want_st).all()
    ke, km, t4 = ecies.DeriveKeysBatch(ks, pts, ctx)
    assert ke.shape == (n, 16) and km.shape == (n, 32) and (t4 == want_st).all()
    assert (ke == want_keys[:, :16]).all() and (km == want_keys[:, 16:]).all()
    seen = set()
    for r in rows:  # one row of each tag through the one-item mirrors
        if r["tag"] in seen:
            continue
        seen.add(r["tag"])
        pt, k = bytes.fromhex(r["point"]), bytes.fromhex(r["scalar"])
        x, y = int.from_bytes(pt[:32], "big"), int.from_bytes(pt[32:], "big")
        got = crypto.ScalarMult(x, y, k.lstrip(b"\0"), ctx)  # scalar.Bytes(): left-padded again inside
        if r["status"] == 0:
            assert got == (int(r["out"][:64], 16), int(r["out"][64:], 16)), r["tag"]
            assert ecies.GenerateShared(k, pt, 16, 16, ctx).hex() == r["shared"], r["tag"]
            assert ecies.GenerateShared(int.from_bytes(k, "big"), (x, y), 16, 16, ctx).hex() == r["shared"]
        else:
            assert got == (None, None), r["tag"]
            err = ecies.ErrSharedKeyIsPointAtInfinity if r["status"] == _lib.ST_INVALID_KEY else ecies.ErrInvalidCurve
            with pytest.raises(err):
                ecies.GenerateShared(k, pt, 16, 16, ctx)
    assert {"bad scalar", "off curve", "bad scalar, off curve", "leading zeros", "x+p"} <= seen
    with pytest.raises(ecies.ErrSharedKeyTooBig):
        ecies.GenerateShared(1, M.pt64(M.G), 32, 32, ctx)
    with pytest.raises(ValueError):
        crypto.ScalarMult(M.GX, M.GY, bytes(33), ctx)
    # ScalarBaseMult, and the reference's own static vector both ways
    a, b = bytes.fromhex(fx["static"]["prv1"]), bytes.fromhex(fx["static"]["prv2"])
    pa, pb = crypto.ScalarBaseMult(a, ctx), crypto.ScalarBaseMult(b, ctx)
    assert pa == M.ec_mul(int.from_bytes(a, "big"), M.G) and pb == M.ec_mul(int.from_bytes(b, "big"), M.G)
    assert ecies.GenerateShared(a, pb, 16, 16, ctx).hex() == fx["static"]["shared"]
    assert ecies.GenerateShared(b, b"\x04" + M.pt64(pa), 16, 16, ctx).hex() == fx["static"]["shared"]
    assert crypto.ScalarBaseMult(b"", ctx) == (None, None) and crypto.ScalarBaseMult(be32(N), ctx) == (None, None)


# ---------------------------------------------------------------- 2. differential
def test_differential_4096(ctx, bulk):
    pts, ks, want_out, want_keys = bulk
    out, st = ctx.secp256k1_scalar_mul_batch(pts, ks)
    assert (st == 0).all()
    assert (out == want_out).all(), np.nonzero((out != want_out).any(axis=1))[0][:10]
    sh, k48, est = ctx.ecdh_batch(pts, ks, want_shared=True, want_keys=True)
    assert (est == 0).all() and (sh == want_out[:, :32]).all()
    assert (k48 == want_keys).all(), np.nonzero((k48 != want_keys).any(axis=1))[0][:10]


def test_ecdh_is_symmetric_4096(ctx):
    rng = random.Random(0x5e55)
    a = u8(b"".join(be32(rng.randrange(1, N)) for _ in range(4096)), 32)
    b = u8(b"".join(be32(rng.randrange(1, N)) for _ in range(4096)), 32)
    pa, _, sa = ctx.pubkey_create_batch(a)
    pb, _, sb = ctx.pubkey_create_batch(b)
    assert (sa == 0).all() and (sb == 0).all()
    x1, k1, s1 = ctx.ecdh_batch(pb[:, 1:], a, want_shared=True, want_keys=True)  # a (bG)
    x2, k2, s2 = ctx.ecdh_batch(pa[:, 1:], b, want_shared=True, want_keys=True)  # b (aG)
    assert (s1 == 0).all() and (s2 == 0).all()
    assert (x1 == x2).all() and x1.any(axis=1).all()
    assert (k1 == k2).all() and (k1 == keys48_of(x1)).all()


# ---------------------------------------------------------------- 3. launch-shape edges
def test_empty_batch_and_argument_errors(ctx):
    from gsv import _lib
    L = _lib.load()
    z64, z32 = np.zeros((0, 64), np.uint8), np.zeros((0, 32), np.uint8)
    out, st = ctx.secp256k1_scalar_mul_batch(z64, z32)
    assert out.shape == (0, 64) and st.shape == (0,)
    sh, k48, st = ctx.ecdh_batch(z64, z32, want_shared=True, want_keys=True)
    assert sh.shape == (0, 32) and k48.shape == (0, 48) and st.shape == (0,)
    h = ctx.handle
    assert L.gsv_secp256k1_scalar_mul_batch(h, None, None, 0, None, None) == 0
    assert L.gsv_secp256k1_scalar_mul_batch_dev(h, None, None, 0, None, None, None) == 0
    assert L.gsv_ecdh_batch(h, None, None, 0, None, None, None) == 0
    assert L.gsv_ecdh_batch_dev(h, None, None, 0, None, None, None, None) == 0
    # n = 0 through the _dev forms writes nothing
    for o in dev_run(ctx, z64, z32):
        assert (o == GUARD).all()
    # argument errors, not faults
    b = np.zeros(64, np.uint8)
    p = b.ctypes.data
    E = _lib.E_INVALID_ARG
    for k in range(4):
        a = [p, p, p, p]
        a[k] = None
        assert L.gsv_secp256k1_scalar_mul_batch(h, a[0], a[1], 1, a[2], a[3]) == E
        assert L.gsv_secp256k1_scalar_mul_batch_dev(h, a[0], a[1], 1, a[2], a[3], None) == E
    for a in ([None, p, p, p, p], [p, None, p, p, p], [p, p, p, p, None], [p, p, None, None, p]):
        assert L.gsv_ecdh_batch(h, a[0], a[1], 1, a[2], a[3], a[4]) == E
        assert L.gsv_ecdh_batch_dev(h, a[0], a[1], 1, a[2], a[3], a[4], None) == E
    assert L.gsv_secp256k1_scalar_mul_batch(h, p, p, 1 << 32, p, p) == E
    assert L.gsv_ecdh_batch(h, p, p, 1 << 32, p, p, p) == E
    with pytest.raises(ValueError):
        ctx.ecdh_batch(z64, z32, want_shared=False, want_keys=False)


@pytest.mark.parametrize("n", SHAPES)
def test_launch_shapes(ctx, bulk, n):
    pts, ks, want_out, want_keys = (a[:n] for a in bulk)
    d_out, d_st, d_sh, d_keys, d_est = dev_run(ctx, pts, ks)
    # the last item against the reference, then all of them; the guard row behind each output untouched
    assert bytes(d_out[n - 1]) == bytes(want_out[n - 1]) and bytes(d_sh[n - 1]) == bytes(want_out[n - 1, :32])
    assert bytes(d_keys[n - 1]) == bytes(want_keys[n - 1])
    assert (d_out[:n] == want_out).all() and (d_sh[:n] == want_out[:, :32]).all() and (d_keys[:n] == want_keys).all()
    assert (d_st[:n] == 0).all() and (d_est[:n] == 0).all()
    for o in (d_out, d_st, d_sh, d_keys, d_est):
        assert (o[n:] == GUARD).all()
    out, st = ctx.secp256k1_scalar_mul_batch(pts, ks)
    sh, k48, est = ctx.ecdh_batch(pts, ks, want_shared=True, want_keys=True)
    assert (out == want_out).all() and (sh == want_out[:, :32]).all() and (k48 == want_keys).all()
    assert (st == 0).all() and (est == 0).all()
    # with an optional output absent nothing is written there, and the other is unchanged
    r = dev_run(ctx, pts, ks, want_shared=False, want_keys=True)
    assert (r[2] == GUARD).all() and (r[3][:n] == want_keys).all() and (r[3][n:] == GUARD).all()
    r = dev_run(ctx, pts, ks, want_shared=True, want_keys=False)
    assert (r[3] == GUARD).all() and (r[2][:n] == want_out[:, :32]).all() and (r[2][n:] == GUARD).all()


# ---------------------------------------------------------------- 5. the scalar and curve rules
def test_scalar_and_curve_rules(ctx, R, bulk):
    from gsv import _lib
    g64 = M.pt64(M.G)
    off = [be32(x) + be32(y) for x, y in M.OFF_CURVE_POINTS]
    assert M.OFF_CURVE_POINTS == ((M.GX, M.GY + 1), (0, 0), (M.GX, P - 1))
    kr = bytes(bulk[1][0])
    # (point, scalar, expected status): each alone in a wave of 63 ordinary lanes
    special = [(g64, be32(k), 11) for k in (0, N, N + 1, 2**256 - 1)]
    special += [(g64, be32(k), 0) for k in (1, N - 1)]
    special += [(pt, kr, 12) for pt in off]
    special += [(off[0], be32(0), 11), (off[1], be32(N), 11), (off[2], be32(2**256 - 1), 11)]
    m = len(special)
    pts, ks, want_out, want_keys = (a[:64 * m].copy() for a in bulk)
    where = [64 * i + i % 64 for i in range(m)]
    for w, (pt, k, s) in zip(where, special):
        pts[w] = np.frombuffer(pt, np.uint8)
        ks[w] = np.frombuffer(k, np.uint8)
        if s == 0:
            rc, o = ref_mul(R, pt, k)
            assert rc == 1
            want_out[w] = np.frombuffer(o, np.uint8)
            want_keys[w] = np.frombuffer(M.kdf_keys(o[:32]), np.uint8)
        else:
            if s == 11:
                assert ref_mul(R, pt, k) == (0, pt)  # the reference's only failure; its buffer untouched
            else:
                assert ref_mul(R, pt, k)[0] == 1     # the divergence: the reference multiplies
            want_out[w] = 0
            want_keys[w] = 0
    want_st = np.zeros(64 * m, np.uint8)
    want_st[where] = [s for _, _, s in special]
    assert _lib.ST_INVALID_KEY == 11 and _lib.ST_INVALID_CURVE == 12
    for via in ("host", "dev"):
        if via == "host":
            out, st = ctx.secp256k1_scalar_mul_batch(pts, ks)
            sh, k48, est = ctx.ecdh_batch(pts, ks, want_shared=True, want_keys=True)
        else:
            out, st, sh, k48, est = (o[:64 * m] for o in dev_run(ctx, pts, ks))
        assert (st == want_st).all() and (est == want_st).all(), (via, np.nonzero(st != want_st)[0])
        assert (out == want_out).all() and (sh == want_out[:, :32]).all() and (k48 == want_keys).all(), via
    # a batch of bad items alone: whole waves of them, every row zero
    bad_pts = u8(b"".join((g64, off[0], off[1], off[2], g64)[i % 5] for i in range(65)), 64)
    bad_ks = u8(b"".join((be32(0), kr, be32(N), kr, be32(2**256 - 1))[i % 5] for i in range(65)), 32)
    want = np.array([(11, 12, 11, 12, 11)[i % 5] for i in range(65)], np.uint8)
    out, st = ctx.secp256k1_scalar_mul_batch(bad_pts, bad_ks)
    sh, k48, est = ctx.ecdh_batch(bad_pts, bad_ks, want_shared=True, want_keys=True)
    assert (st == want).all() and (est == want).all()
    assert not out.any() and not sh.any() and not k48.any()


# ---------------------------------------------------------------- 6. the ladder's edges
def test_ladder_edges(ctx, R):
    """every edge scalar on every edge point, against the reference: the four parity cases of
    glv_make_odd, zero GLV halves, the top-digit start"""
    pairs = [(M.pt64(pt), be32(k)) for pt in M.ladder_points() for k in M.LADDER_SCALARS]
    assert len(pairs) == 120
    want = []
    for pt, k in pairs:
        rc, o = ref_mul(R, pt, k)
        assert rc == 1
        want.append(o)
    want = u8(b"".join(want), 64)
    pts, ks = u8(b"".join(p for p, _ in pairs), 64), u8(b"".join(k for _, k in pairs), 32)
    out, st = ctx.secp256k1_scalar_mul_batch(pts, ks)
    assert (st == 0).all(), np.nonzero(st)[0]
    assert (out == want).all(), [(i // 20, hex(M.LADDER_SCALARS[i % 20])) for i in np.nonzero((out != want).any(axis=1))[0]]
    sh, k48, est = ctx.ecdh_batch(pts, ks, want_shared=True, want_keys=True)
    assert (est == 0).all() and (sh == want[:, :32]).all() and (k48 == keys48_of(want[:, :32])).all()
    # all four parity cases of glv_make_odd occur among them (tests/secp_glv_model.py reads the device's constants)
    import secp_glv_model as GM
    assert {GM.make_odd(*GM.split_lambda(k))[2] for k in M.LADDER_SCALARS} == {"v1", "v2", "v3", "none"}


# ---------------------------------------------------------------- 7. coordinates >= p
def test_unreduced_coordinates(ctx, R):
    cases = M.unreduced_cases()
    assert [t for t, _, _ in cases] == golden("secp_ecdh.json")["unreduced"] and cases[0][0] == "x+p"
    rng = random.Random(77)
    for tag, raw, red in cases:
        assert raw != red
        ks = u8(b"".join(be32(rng.randrange(1, N)) for _ in range(8)), 32)
        o_raw, s_raw = ctx.secp256k1_scalar_mul_batch(u8(raw * 8, 64), ks)
        o_red, s_red = ctx.secp256k1_scalar_mul_batch(u8(red * 8, 64), ks)
        assert (s_raw == 0).all() and (s_red == 0).all() and (o_raw == o_red).all(), tag
        for i in range(8):
            assert ref_mul(R, raw, bytes(ks[i])) == (1, bytes(o_raw[i])), tag
        sh, _, est = ctx.ecdh_batch(u8(raw * 8, 64), ks)
        assert (est == 0).all() and (sh == o_red[:, :32]).all()


# ---------------------------------------------------------------- 8. leading zeros
def test_leading_zero_shared_secret(ctx, R):
    from gsv import ecies
    pt, k = M.leading_zero_case(random.Random(88))
    want = bytes(31) + b"\x01"
    assert ref_mul(R, pt, k)[1][:32] == want
    sh, k48, st = ctx.ecdh_batch(u8(pt, 64), u8(k, 32), want_shared=True, want_keys=True)
    assert st[0] == 0 and bytes(sh[0]) == want and bytes(k48[0]) == M.kdf_keys(want)
    assert ecies.GenerateShared(k, pt, 16, 16, ctx) == want


# ---------------------------------------------------------------- 9. secret hygiene
def test_staged_secrets_are_wiped(ctx):
    """after each host form returns, the arena's secret regions (first and contiguous from offset 0:
    tests/test_ecdh_stage_host.py) hold nothing; the public points behind them still hold their input, so
    the read looks at the arena this call staged in"""
    def al(b):
        return (b + 255) // 256 * 256
    n = 300
    ks = np.full((n, 32), 0xA5, np.uint8)
    pts = u8(M.pt64(M.G) * n, 64)
    out, st = ctx.secp256k1_scalar_mul_batch(pts, ks)
    assert (st == 0).all() and out.any(axis=1).all()
    secret = al(n * 32) + al(n * 64)
    assert not ctx._arena_read(0, secret).any(), "staged scalars or products left in the arena"
    assert (ctx._arena_read(secret, n * 64).reshape(n, 64) == pts).all()
    for ws, wk in ((True, True), (True, False), (False, True)):
        sh, k48, st = ctx.ecdh_batch(pts, ks, want_shared=ws, want_keys=wk)
        assert (st == 0).all() and (sh is None or sh.any(axis=1).all()) and (k48 is None or k48.any(axis=1).all())
        secret = al(n * 32) + (al(n * 32) if ws else 0) + (al(n * 48) if wk else 0)
        assert not ctx._arena_read(0, secret).any(), "staged keys, shared secrets or derived keys left in the arena"
        assert (ctx._arena_read(secret, n * 64).reshape(n, 64) == pts).all()


# ---------------------------------------------------------------- 10. capture
def test_dev_form_is_capturable(ctx, bulk):
    import torch
    from gsv import _lib
    dev = torch.device("cuda", ctx.device)
    n = 257
    pts, ks, want_out, want_keys = (a[:n] for a in bulk)
    d_pt = torch.from_numpy(np.array(pts)).to(dev)
    d_k = torch.from_numpy(np.array(ks)).to(dev)
    d_sh = torch.full((n, 32), GUARD, dtype=torch.uint8, device=dev)
    d_keys = torch.full((n, 48), GUARD, dtype=torch.uint8, device=dev)
    d_st = torch.full((n,), GUARD, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    cs = torch.cuda.Stream()
    # one launch per call, timed under K_ECRECOVER
    ctx.set_timing(True)
    try:
        ctx.reset_timing()
        ctx.ecdh_batch_dev(d_pt, d_k, d_sh, d_keys, d_st, stream=cs)
        cs.synchronize()
        ms, launches = ctx.kernel_time(_lib.K_ECRECOVER)
        assert launches == 1 and ms > 0
    finally:
        ctx.set_timing(False)
        ctx.reset_timing()
    assert (d_sh.cpu().numpy() == want_out[:, :32]).all() and (d_keys.cpu().numpy() == want_keys).all()
    # captured on an explicit stream (nothing allocated, nothing synchronised inside), replayed twice
    g = torch.cuda.CUDAGraph()
    shapes_before = ctx.prepared_shapes()
    with torch.cuda.graph(g, stream=cs):
        ctx.ecdh_batch_dev(d_pt, d_k, d_sh, d_keys, d_st, stream=cs)
    assert ctx.prepared_shapes() == shapes_before
    for _ in range(2):
        for t in (d_sh, d_keys, d_st):
            t.fill_(GUARD)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert (d_sh.cpu().numpy() == want_out[:, :32]).all() and (d_keys.cpu().numpy() == want_keys).all()
        assert (d_st.cpu().numpy() == 0).all()
