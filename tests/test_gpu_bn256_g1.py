"""GPU tests of the batched bn256Add / bn256ScalarMul precompiles (gsv_bn256_add_batch,
gsv_bn256_scalar_mul_batch and their _dev forms; core/vm/contracts.go:274-312).  Expectations come
from the committed reference vectors, the CPU oracle (oracle.bn256_g1_mul) and the pure-Python model
(tests/bn254_g1_py.py) — never from the code under test."""
import contextlib
import os
import random

import numpy as np
import pytest

import bn254_g1_py as M
from bn254_py import P, R
from conftest import golden

pytestmark = pytest.mark.gpu

OK, BAD = 0, 9  # GSV_ST_OK, GSV_ST_BN_BAD_INPUT
Z64 = bytes(64)


def be(x):
    return int(x).to_bytes(32, "big")


def rows(out):
    return [bytes(r) for r in out]


class bitserial:
    """the launcher's bit-serial multiplication kernel for the calls inside the block"""

    def __enter__(self):
        os.environ["GSV_BN_G1_BITSERIAL"] = "1"

    def __exit__(self, *a):
        del os.environ["GSV_BN_G1_BITSERIAL"]


def neg64(pt: bytes) -> bytes:
    y = int.from_bytes(pt[32:], "big")
    return pt[:32] + be((P - y) % P)


@pytest.fixture(scope="module")
def ref(oracle):
    """Computed once, never modified: 4,097 points a_i G and the differential cases built on them."""
    rng = random.Random(20240608)
    a = [rng.randrange(1, R) for _ in range(4097)]
    pts = [oracle.bn256_g1_mul(x) for x in a]
    # ---- multiplication: point i, scalar uniform over 256 bits; every 64th small; every 97th point
    # infinity or malformed
    mul_in, mul_exp, mul_st = [], [], []
    for i in range(4096):
        k = rng.getrandbits(20) if i % 64 == 63 else rng.getrandbits(256)
        pt = pts[i]
        if i % 97 == 96:
            kind = (i // 97) % 3
            pt = Z64 if kind == 0 else pt[:63] + bytes([pt[63] ^ 1]) if kind == 1 else be(P) + pt[32:]
        e = oracle.bn256_g1_mul(k, pt)
        mul_in.append(pt + be(k))
        mul_exp.append(Z64 if e is None else e)
        mul_st.append(BAD if e is None else OK)
    # ---- addition: a_i G + b G == (a_i + b mod r) G, with b = a_i (doubling) and b = -a_i mixed in
    add_in, add_exp = [], []
    for i in range(4096):
        if i % 16 == 5:
            add_in.append(pts[i] + pts[i])
            add_exp.append(oracle.bn256_g1_mul(2 * a[i] % R))
        elif i % 16 == 11:
            add_in.append(pts[i] + neg64(pts[i]))
            add_exp.append(oracle.bn256_g1_mul(0))
        else:
            add_in.append(pts[i] + pts[i + 1])
            add_exp.append(oracle.bn256_g1_mul((a[i] + a[i + 1]) % R))
    assert add_exp[11] == Z64
    return {"a": a, "pts": pts, "mul_in": mul_in, "mul_exp": mul_exp, "mul_st": mul_st, "add_in": add_in,
            "add_exp": add_exp}


# ---------------------------------------------------------------- 4. reference vectors
def test_reference_vectors(ctx):
    from gsv import bn256
    add = golden("bn256_g1.json")["add"]
    mul = golden("bn256.json")["scalar_mul"]
    assert len(add) == 16 and len(mul) == 18
    for vec, batch, cls in ((add, ctx.bn256_add_batch, bn256.Bn256Add), (mul, ctx.bn256_scalar_mul_batch,
                                                                        bn256.Bn256ScalarMul)):
        out, st = batch([bytes.fromhex(r["input"]) for r in vec])
        for r, o, s in zip(vec, rows(out), st):
            if r["expected"]:
                assert s == OK and o.hex() == r["expected"], r["name"]
                assert cls().Run(bytes.fromhex(r["input"]), ctx).hex() == r["expected"], r["name"]
            else:  # a row whose expected result is the error
                assert s == BAD and o == Z64, r["name"]
                with pytest.raises(bn256.ErrMalformedPoint):
                    cls().Run(bytes.fromhex(r["input"]), ctx)
    # the conveniences, and the error the reference returns for a malformed point
    g = M.g1_encode(M.G)
    assert bn256.G1Add(g, g, ctx) == M.g1_encode(M.g1_mul(M.G, 2))
    assert bn256.G1ScalarMult(g, 7, ctx) == M.g1_encode(M.g1_mul(M.G, 7))
    for cls, tail in ((bn256.Bn256Add, g), (bn256.Bn256ScalarMul, be(0))):
        with pytest.raises(bn256.ErrMalformedPoint):
            cls().Run(be(1) + be(3) + tail, ctx)


# ---------------------------------------------------------------- 5. addition edges
def test_add_edges_one_batch_of_65(ctx, ref, oracle):
    a, pts = ref["a"], ref["pts"]
    p, q = pts[0], pts[1]
    pq = oracle.bn256_g1_mul((a[0] + a[1]) % R)
    p2 = oracle.bn256_g1_mul(2 * a[0] % R)
    off = p[:63] + bytes([p[63] ^ 1])  # y +- 1: off the curve
    cases = [
        ("P + inf", p + Z64, p), ("inf + P", Z64 + p, p), ("inf + inf", Z64 + Z64, Z64), ("P + P", p + p, p2),
        ("P + (-P)", p + neg64(p), Z64),
        ("x = p", be(P) + p[32:] + q, None), ("y = p", p[:32] + be(P) + q, None),
        ("x = p + 1", be(P + 1) + p[32:] + q, None), ("x = 2^256 - 1", be(2**256 - 1) + p[32:] + q, None),
        ("(0, 1)", be(0) + be(1) + q, None), ("(1, 3)", be(1) + be(3) + q, None),
        ("(p, 0) is not infinity", be(P) + be(0) + q, None), ("(0, p) is not infinity", q + be(0) + be(P), None),
        ("bad + good", off + q, None), ("good + bad", q + off, None),
        ("empty", b"", Z64), ("64 bytes", p, p), ("200 bytes", p + q + bytes([0xAB]) * 72, pq),
    ]
    assert len(cases[-1][1]) == 200 and len(cases[-2][1]) == 64
    # fill to 65 items (a full wave and a one-lane tail) with sums from the shared reference
    k = 65 - len(cases)
    cases += [("sum %d" % i, ref["add_in"][i], ref["add_exp"][i]) for i in range(k)]
    assert len(cases) == 65
    out, st = ctx.bn256_add_batch([c[1] for c in cases])
    for (name, inp, want), o, s in zip(cases, rows(out), st):
        assert want == M.run_add(inp), name  # the expectation agrees with the independent model
        if want is None:
            assert s == BAD and o == Z64, name
        else:
            assert s == OK and o == want, name


# ---------------------------------------------------------------- 6. multiplication edges
def test_mul_edges(ctx, ref, oracle):
    g = M.g1_encode(M.G)
    p = ref["pts"][2]
    ins, want = [], []
    for pt in (g, p):
        for k in M.EDGE_SCALARS:
            ins.append(pt + be(k))
            want.append(oracle.bn256_g1_mul(k, pt))
    # r - 1 gives -P, r gives infinity
    i0 = M.EDGE_SCALARS.index(R - 1)
    assert want[len(M.EDGE_SCALARS) + i0] == neg64(p) and want[i0 + 1] == Z64
    ins += [Z64 + be(5), be(1) + be(3) + be(0), be(P) + be(2) + be(0), b"", p, (p + be(2**255 + 12345))[:95],
            p + be(7) + b"\x01"]
    want += [Z64, None, None, Z64, Z64, oracle.bn256_g1_mul((2**255 + 12345) >> 8 << 8, p), oracle.bn256_g1_mul(7, p)]
    assert [len(x) for x in ins[-4:]] == [0, 64, 95, 97]
    for bs in (False, True):
        with (bitserial() if bs else contextlib.nullcontext()):
            out, st = ctx.bn256_scalar_mul_batch(ins)
        for i, (inp, w, o, s) in enumerate(zip(ins, want, rows(out), st)):
            assert w == M.run_mul(inp), i  # oracle and model agree on the expectation
            if w is None:
                assert s == BAD and o == Z64, (i, bs)
            else:
                assert s == OK and o == w, (i, bs)


# ---------------------------------------------------------------- 7. differential
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096])
def test_mul_differential(ctx, ref, n):
    want_o, want_s = ref["mul_exp"][:n], ref["mul_st"][:n]
    out, st = ctx.bn256_scalar_mul_batch(ref["mul_in"][:n])
    assert list(st) == want_s
    assert rows(out) == want_o
    with bitserial():
        out2, st2 = ctx.bn256_scalar_mul_batch(ref["mul_in"][:n])
    assert list(st2) == want_s and rows(out2) == want_o


def test_add_differential(ctx, ref):
    out, st = ctx.bn256_add_batch(ref["add_in"])
    assert not st.any()
    assert rows(out) == ref["add_exp"]


# ---------------------------------------------------------------- 8. device-resident composition
def test_dev_scalar_mul_feeds_pairing(ctx, oracle):
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = random.Random(77)
    n = 64
    a = [rng.randrange(1, R) for _ in range(n)]
    b = [rng.randrange(1, R) for _ in range(n)]
    g = M.g1_encode(M.G)
    recs = [g + be(x) for x in a] + [g + be((R - x * y % R) % R) for x, y in zip(a, b)]
    g2 = np.frombuffer(b"".join(oracle.bn256_g2_mul(y) for y in b), np.uint8).reshape(n, 128)
    q1 = np.frombuffer(oracle.bn256_g2_mul(1) * n, np.uint8).reshape(n, 128)
    off = np.arange(n + 1, dtype=np.uint64) * 384
    ctx.pairing_prepare(off)
    (s,) = ctx.pipeline_streams(1)
    try:
        d_in = torch.from_numpy(np.frombuffer(b"".join(recs), np.uint8).reshape(2 * n, 96).copy()).to(dev)
        d_bq, d_q = torch.from_numpy(g2.copy()).to(dev), torch.from_numpy(q1.copy()).to(dev)
        d_out = torch.empty((2 * n, 64), dtype=torch.uint8, device=dev)
        d_st = torch.empty((2 * n,), dtype=torch.uint8, device=dev)
        d_pin = torch.empty((n, 384), dtype=torch.uint8, device=dev)
        d_ver = torch.empty((n,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

        def run():
            ctx.bn256_scalar_mul_batch_dev(d_in, d_out, d_st, stream=s)
            with torch.cuda.stream(s):
                d_pin[:, 0:64] = d_out[:n]
                d_pin[:, 64:192] = d_bq
                d_pin[:, 192:256] = d_out[n:]
                d_pin[:, 256:384] = d_q
            ctx.pairing_check_batch_dev(d_pin.view(-1), off, d_ver, stream=s, prepare=False)
            s.synchronize()
            return d_ver.cpu().numpy()

        assert (run() == 1).all()  # GSV_PAIRING_TRUE
        assert not d_st.cpu().numpy().any()
        h_out, h_st = ctx.bn256_scalar_mul_batch(recs)
        assert not h_st.any() and (d_out.cpu().numpy() == h_out).all()
        assert rows(h_out[:n]) == [oracle.bn256_g1_mul(x) for x in a]
        # perturb one scalar: that check turns FALSE, the others stay TRUE
        bad = list(recs)
        bad[n + 17] = g + be(((R - a[17] * b[17] % R) + 1) % R)
        d_in.copy_(torch.from_numpy(np.frombuffer(b"".join(bad), np.uint8).reshape(2 * n, 96).copy()))
        torch.cuda.synchronize()
        v = run()
        assert v[17] == 0 and (np.delete(v, 17) == 1).all()
    finally:
        torch.cuda.synchronize()
        ctx.destroy_streams([s])


# ---------------------------------------------------------------- 9. timing id, empty batch
def test_kernel_time_and_empty_batch(ctx, ref):
    import torch
    from gsv import _lib
    dev = torch.device("cuda", ctx.device)
    ctx.set_timing(True)
    try:
        ctx.reset_timing()
        ctx.bn256_add_batch(ref["add_in"][:3])
        assert ctx.kernel_time(_lib.K_BN_G1)[1] == 1
        ctx.bn256_scalar_mul_batch(ref["mul_in"][:3])
        ms, launches = ctx.kernel_time(_lib.K_BN_G1)
        assert launches == 2 and ms > 0
        # n = 0: success, nothing launched, on all four entry points
        out, st = ctx.bn256_add_batch([])
        assert out.shape == (0, 64) and st.shape == (0,)
        out, st = ctx.bn256_scalar_mul_batch([])
        assert out.shape == (0, 64) and st.shape == (0,)
        L = _lib.load()
        assert L.gsv_bn256_add_batch(ctx.handle, None, None, 0, None, None) == 0
        assert L.gsv_bn256_scalar_mul_batch(ctx.handle, None, None, 0, None, None) == 0
        e = torch.empty((0, 128), dtype=torch.uint8, device=dev)
        o = torch.empty((0, 64), dtype=torch.uint8, device=dev)
        z = torch.empty((0,), dtype=torch.uint8, device=dev)
        ctx.bn256_add_batch_dev(e, o, z)
        ctx.bn256_scalar_mul_batch_dev(torch.empty((0, 96), dtype=torch.uint8, device=dev), o, z)
        torch.cuda.synchronize()
        assert ctx.kernel_time(_lib.K_BN_G1)[1] == 2
    finally:
        ctx.set_timing(False)
        ctx.reset_timing()
