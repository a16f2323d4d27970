"""GPU parity of batched ECDSA verification with a known key (k_ecverify) and of public-key parsing
(k_pubkey_parse).  Expected verdicts come from the Python-integer model (tests/secp_verify_model.py) for
every special case, and for the bulk from the identity with recovery (verify is true <=> the key parses,
s <= n/2, and some recid makes the oracle's ecrecover return the parsed key).

The exceptional cases of the kernel's final add u1 G + u2 P and where each is reached:
  u1 G = O (u1 = 0; msg = 0 and msg = n)         test_chosen_scalars, test_final_add_cases (the r + n item)
  u1 G = u2 P (the doubling)                      test_final_add_cases
  u1 G = -u2 P (the identity: invalid)            test_final_add_cases
  r < p - n and X_x = r + n                       test_final_add_cases
  the ladder's own doubling (U2_DOUBLING)         test_chosen_scalars
u2 P = O cannot be built for a key of order n; the kernel honours the ladder's flag all the same."""
import random

import numpy as np
import pytest

import secp_glv_model as M
import secp_verify_model as V
from conftest import golden

pytestmark = pytest.mark.gpu
N, LAM = M.N, M.LAMBDA
U2_DOUBLING = (-26 * LAM) % N  # test_gpu_secp256k1_scalars.py: the last lambda add finds acc == P


def u8(b, width):
    return np.frombuffer(bytes(b), np.uint8).reshape(-1, width)


def run(ctx, items):
    """items [(msg32, sig64, key)] -> ok (n,) through the host entry point"""
    msgs = u8(b"".join(m for m, _, _ in items), 32)
    sigs = u8(b"".join(s for _, s, _ in items), 64)
    return ctx.ecdsa_verify_batch(msgs, sigs, [k for _, _, k in items])


def device_layout(keys):
    """the _dev forms' layout: rows (n, 65) zero-padded, and the length bytes (33, 65, else 0)"""
    rows = np.zeros((len(keys), 65), np.uint8)
    lens = np.zeros(len(keys), np.uint8)
    for i, k in enumerate(keys):
        if len(k) in (33, 65):
            rows[i, :len(k)] = np.frombuffer(k, np.uint8)
            lens[i] = len(k)
    return rows, lens


@pytest.fixture(scope="module")
def ordinary(ctx):
    """valid items from the synthetic signer: (msg32, sig64, uncompressed key)"""
    msg, sig, pub, _ = ctx.synth_sign(seed=4242, n=49152, want_pub=True, want_addr=False)
    return [(bytes(msg[i]), bytes(sig[i, :64]), bytes(pub[i])) for i in range(len(msg))]


def among(ctx, ordinary, items):
    """each item in a wave of its own among 63 ordinary lanes (lane i % 64 of wave i): ok of the items"""
    assert 64 * len(items) <= len(ordinary)
    batch = list(ordinary[:64 * len(items)])
    where = [64 * i + i % 64 for i in range(len(items))]
    for w, it in zip(where, items):
        batch[w] = it
    ok = run(ctx, batch)
    rest = np.ones(len(batch), bool)
    rest[where] = False
    assert (ok[rest] == 1).all()  # the ordinary lanes are untouched by their neighbour
    return ok[where]


def alone(ctx, items):
    """each item as a batch of one: a lone lane in a lone wave"""
    return np.array([run(ctx, [it])[0] for it in items], np.uint8)


# ---------------------------------------------------------------- 1. the reference's vectors
def test_fixture_vectors(ctx):
    from gsv import crypto
    g = golden("secp_verify.json")
    full, comp = bytes.fromhex(g["testpubkey"]), bytes.fromhex(g["testpubkeyc"])
    msg, sig = bytes.fromhex(g["testmsg"]), bytes.fromhex(g["testsig"])[:-1]
    pt = V.parse_pubkey(full)
    wrong = bytearray(full)
    wrong[10] = (wrong[10] + 1) & 0xFF
    m = g["malleable"]
    items = [(msg, sig, V.encode(pt, f)) for f in (4, 2, 6)] + [(msg, sig, bytes(wrong))] + \
            [(bytes.fromhex(m["msg"]), bytes.fromhex(m["sig"]), bytes.fromhex(m["key"]))]
    assert items[0][2] == full and items[1][2] == comp and items[2][2][0] in (6, 7)
    want = [V.verify(*it) for it in items]
    assert want == [True, True, True, False, False]
    assert list(run(ctx, items)) == want
    assert list(alone(ctx, items)) == want
    # through the crypto mirror, with its length rules
    assert crypto.VerifySignature(full, msg, sig, ctx) is True
    assert crypto.VerifySignature(comp, msg, sig, ctx) is True
    assert crypto.VerifySignature(bytes(wrong), msg, sig, ctx) is False
    got = crypto.VerifySignatureBatch([full, b"", comp, full, full], [msg, msg, msg, b"", msg],
                                      [sig, sig, sig, sig, sig + b"\x01\x02\x03"], ctx)
    assert list(got) == [True, False, True, False, False]
    assert crypto.DecompressPubkey(comp, ctx) == full and crypto.CompressPubkey(full, ctx) == comp


# ---------------------------------------------------------------- 2. rejections
@pytest.fixture(scope="module")
def valid_item():
    rng = random.Random(0x7e52)
    d, k = rng.randrange(1, N), rng.randrange(1, N)
    pt = M.ec_mul(d, M.G)
    msg = bytes(rng.getrandbits(8) for _ in range(32))
    return msg, V.sign(d, msg, k), pt


def test_rejections(ctx, ordinary, valid_item):
    msg, sig, pt = valid_item
    cases = V.rejection_cases(msg, sig, pt)
    names = [c[0] for c in cases]
    for must in ("msg bit", "r bit", "s bit", "key x bit", "high s", "r = 0", "s = 0", "hybrid wrong parity",
                 "prefix 05", "prefix 00", "x = p", "y = p", "x > p", "off the curve", "compressed non-residue",
                 "65 bytes with prefix 02", "33 bytes with prefix 04") + tuple("length %d" % n for n in V.BAD_LENGTHS):
        assert must in names, must
    items = [(msg, sig, V.encode(pt, f)) for f in (4, 2, 6)] + [c[1:] for c in cases]
    want = np.array([V.verify(*it) for it in items], np.uint8)
    assert want[:3].all() and not want[3:].any()
    got = run(ctx, items)
    assert (got == want).all(), [names[i - 3] for i in np.nonzero(got != want)[0]]
    got = among(ctx, ordinary, items)
    assert (got == want).all(), [names[i - 3] for i in np.nonzero(got != want)[0]]


# ---------------------------------------------------------------- 3. chosen scalars
@pytest.fixture(scope="module")
def chosen():
    """[(label, msg32, sig64, key)]: verifications that compute u1 G + u2 P for chosen (u1, u2).  The
    model's exceptional u2 (the ladder's doubling) with every u1 of the list below; a + b lambda for
    |a|, |b| <= 3, the centres of the near-constant family (n - 1, n/2, 2^128, 2^129, +-lambda, the lattice
    vectors, t n/M) and the neighbours of n/2, 2^128 and +-lambda, with u1 rotating through that list.  u1: 0 (as msg = 0 and as msg = n), 1, a random value, and
    d 2^(20 w) for d = 1 and 2^20 - 1 in every window (below n)."""
    rng = random.Random(0xc405e)
    exc = sorted(M.exceptional_scalars())
    assert U2_DOUBLING in exc
    edges = [d << (M.COMB_BITS * w) for w in range(M.COMB_WINDOWS) for d in (1, (1 << M.COMB_BITS) - 1)]
    u1s = [0, 1, rng.randrange(1, N)] + [e for e in edges if e < N]
    assert len(u1s) >= 2 * M.COMB_WINDOWS + 1
    pairs = [(u1, u2) for u2 in exc for u1 in u1s]
    fam = [u for u, _, _ in M.small_family(3)] + M.near_constant_family(0)
    fam += [(c + e) % N for c in (N // 2, 1 << 128, LAM, N - LAM) for e in (-2, -1, 1, 2)]
    pairs += [(u1s[i % len(u1s)], u2) for i, u2 in enumerate(fam)]
    out = []
    for i, (u1, u2) in enumerate(pairs):
        pt, msg, sig = V.point_for(u1, u2, seed=rng.randrange(1, 1 << 255))
        key = V.encode(pt, (4, 2, 6)[i % 3])
        out.append(("u1=%x u2=%x" % (u1, u2), msg, sig, key))
        if u1 == 0:
            assert msg == bytes(32)
            out.append(("u1=0 as msg=n u2=%x" % u2, V.be32(N), sig, key))
    return out


def test_chosen_scalars(ctx, ordinary, chosen):
    items = [c[1:] for c in chosen]
    assert 250 < len(items) <= 768
    for c in chosen:
        assert V.verify(*c[1:]), c[0]  # the model: every item is valid
    got = among(ctx, ordinary, items)
    assert got.all(), [chosen[i][0] for i in np.nonzero(got == 0)[0]]
    got = alone(ctx, items)
    assert got.all(), [chosen[i][0] for i in np.nonzero(got == 0)[0]]
    got = run(ctx, items)  # together: whole waves take the rare branches
    assert got.all(), [chosen[i][0] for i in np.nonzero(got == 0)[0]]


# ---------------------------------------------------------------- 4. the final add
def test_final_add_cases(ctx, ordinary):
    rng = random.Random(0xf1ad)
    cases = []  # (label, item, expected)
    for _ in range(3):
        d, k = rng.randrange(1, N), rng.randrange(1, N)
        pt = M.ec_mul(d, M.G)
        r = M.ec_mul(k, M.G)[0] % N
        # u1 G = u2 P: u1 = u2 d via msg = r d; then X = 2 u2 P = (2 r d / s) G, which is +-k G for
        # s = 2 r d / k, taken low
        s = 2 * r * d * pow(k, -1, N) % N
        s = N - s if s > M.HALF_N else s
        for f in (4, 2, 6):
            cases.append(("doubling", (V.be32(r * d % N), V.be32(r) + V.be32(s), V.encode(pt, f)), True))
        # u1 G = -u2 P: msg = -r d, any s
        for s2 in (s, 1, rng.randrange(1, M.HALF_N)):
            cases.append(("cancellation", (V.be32(-r * d % N), V.be32(r) + V.be32(s2), V.encode(pt, 4)), False))
    # r + n: the key is the first point with x > n (secp_verify_model.first_x_above_n says why not x = n),
    # msg = 0 and r = s = x - n: u1 = 0, u2 = 1, X = P
    pt = V.first_x_above_n()
    r = pt[0] - N
    assert 0 < r < M.P - N
    for f in (4, 2, 6):
        for p in (pt, (pt[0], M.P - pt[1])):
            cases.append(("r + n", (bytes(32), V.be32(r) + V.be32(r), V.encode(p, f)), True))
            cases.append(("r + n + 1", (bytes(32), V.be32(r + 1) + V.be32(r + 1), V.encode(p, f)), False))
    cases.append(("x = n", (bytes(32), bytes(64), V.encode(M.lift_x(N, 0), 4)), False))
    items = [c[1] for c in cases]
    want = np.array([c[2] for c in cases], np.uint8)
    assert [V.verify(*it) for it in items] == [c[2] for c in cases]
    for got in (among(ctx, ordinary, items), alone(ctx, items), run(ctx, items)):
        assert (got == want).all(), [cases[i][0] for i in np.nonzero(got != want)[0]]


# ---------------------------------------------------------------- 5, 6. shapes and the bulk
@pytest.fixture(scope="module")
def bulk(oracle):
    """4,096 seeded items (even: valid, odd: one mutation; keys compressed and uncompressed in turn) and
    their verdicts by the identity with the oracle's recovery"""
    n = 4096
    items = V.bulk_items(oracle, 0xb01d, n)
    msgs = np.repeat(u8(b"".join(it[0] for it in items), 32), 4, axis=0)
    sigs = np.zeros((4 * n, 65), np.uint8)
    sigs[:, :64] = np.repeat(u8(b"".join(it[1] for it in items), 64), 4, axis=0)
    sigs[:, 64] = np.tile(np.arange(4, dtype=np.uint8), n)
    opub, ost = oracle.ecrecover_batch(msgs, sigs, threads=16)
    want = np.zeros(n, np.uint8)
    for i, (msg, sig, key) in enumerate(items):
        pub, ok = V.reencode(key)
        if ok and int.from_bytes(sig[32:], "big") <= M.HALF_N:
            want[i] = any(ost[4 * i + v] == 0 and bytes(opub[4 * i + v]) == pub for v in range(4))
    assert want[0::2].all() and not want[1::2].any()
    return items, want


def test_bulk(ctx, bulk):
    items, want = bulk
    got = run(ctx, items)
    assert (got == want).all(), np.nonzero(got != want)[0][:10]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_shapes_host_dev_graph(ctx, bulk, n):
    import torch
    dev = torch.device("cuda", ctx.device)
    items, want = bulk[0][:n], bulk[1][:n]
    host = run(ctx, items)
    assert (host == want).all(), np.nonzero(host != want)[0][:10]
    rows, lens = device_layout([k for _, _, k in items])
    d_msg = torch.from_numpy(u8(b"".join(m for m, _, _ in items), 32).copy()).to(dev)
    d_sig = torch.from_numpy(u8(b"".join(s for _, s, _ in items), 64).copy()).to(dev)
    d_rows, d_lens = torch.from_numpy(rows).to(dev), torch.from_numpy(lens).to(dev)
    d_ok = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    d_out = torch.full((n, 65), 9, dtype=torch.uint8, device=dev)
    d_pok = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    cs = torch.cuda.Stream()
    ctx.ecdsa_verify_batch_dev(d_msg, d_sig, d_rows, d_lens, d_ok, stream=cs)
    ctx.pubkey_parse_batch_dev(d_rows, d_lens, d_out, d_pok, stream=cs)
    cs.synchronize()
    assert d_ok.cpu().numpy().tobytes() == host.tobytes()
    h_out, h_pok = ctx.pubkey_parse_batch([k for _, _, k in items])
    assert d_out.cpu().numpy().tobytes() == h_out.tobytes() and d_pok.cpu().numpy().tobytes() == h_pok.tobytes()
    # captured on an explicit stream (nothing allocated, nothing synchronised inside), replayed once
    d_ok.fill_(9)
    d_out.fill_(9)
    d_pok.fill_(9)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    shapes_before = ctx.prepared_shapes()
    with torch.cuda.graph(g, stream=cs):
        ctx.ecdsa_verify_batch_dev(d_msg, d_sig, d_rows, d_lens, d_ok, stream=cs)
        ctx.pubkey_parse_batch_dev(d_rows, d_lens, d_out, d_pok, stream=cs)
    assert ctx.prepared_shapes() == shapes_before
    g.replay()
    torch.cuda.synchronize()
    assert d_ok.cpu().numpy().tobytes() == host.tobytes()
    assert d_out.cpu().numpy().tobytes() == h_out.tobytes() and d_pok.cpu().numpy().tobytes() == h_pok.tobytes()


def test_empty_batch_and_timing_id(ctx, bulk):
    from gsv import _lib
    L = _lib.load()
    assert ctx.ecdsa_verify_batch(np.zeros((0, 32), np.uint8), np.zeros((0, 64), np.uint8), []).shape == (0,)
    out, ok = ctx.pubkey_parse_batch([])
    assert out.shape == (0, 65) and ok.shape == (0,)
    assert L.gsv_ecdsa_verify_batch(ctx.handle, None, None, None, None, 0, None) == 0
    assert L.gsv_ecdsa_verify_batch_dev(ctx.handle, None, None, None, None, 0, None, None) == 0
    assert L.gsv_pubkey_parse_batch(ctx.handle, None, None, 0, None, None) == 0
    assert L.gsv_pubkey_parse_batch_dev(ctx.handle, None, None, 0, None, None, None) == 0
    # descending offsets and a missing key buffer are argument errors, not faults
    msg, sig = (np.zeros((2, w), np.uint8) for w in (32, 64))
    ok2 = np.zeros(2, np.uint8)
    p = lambda a: a.ctypes.data  # noqa: E731
    bad = np.array([65, 0, 65], np.uint64)
    keys = np.zeros(130, np.uint8)
    assert L.gsv_ecdsa_verify_batch(ctx.handle, p(msg), p(sig), p(keys), p(bad), 2, p(ok2)) == _lib.E_INVALID_ARG
    good = np.array([0, 65, 130], np.uint64)
    assert L.gsv_ecdsa_verify_batch(ctx.handle, p(msg), p(sig), None, p(good), 2, p(ok2)) == _lib.E_INVALID_ARG
    assert L.gsv_pubkey_parse_batch(ctx.handle, None, p(good), 2, p(keys), p(ok2)) == _lib.E_INVALID_ARG
    assert L.gsv_ecdsa_verify_batch(ctx.handle, p(msg), p(sig), p(keys), p(good), 1 << 32, p(ok2)) == _lib.E_INVALID_ARG
    ctx.set_timing(True)
    try:
        ctx.reset_timing()
        run(ctx, bulk[0][:3])
        ctx.pubkey_parse_batch([bulk[0][0][2]])
        ms, launches = ctx.kernel_time(_lib.K_ECRECOVER)
        assert launches == 2 and ms > 0
    finally:
        ctx.set_timing(False)
        ctx.reset_timing()


# ---------------------------------------------------------------- 7. the parse kernel
def test_pubkey_parse(ctx, oracle, valid_item):
    from gsv import crypto
    rng = random.Random(0x9a75e)
    full = [oracle.secp_pubkey(V.be32(rng.randrange(1, N))) for _ in range(64)]
    pts = [(int.from_bytes(k[1:33], "big"), int.from_bytes(k[33:], "big")) for k in full]
    want = u8(b"".join(full), 65)
    for form in (2, 6, 4):
        out, ok = ctx.pubkey_parse_batch([V.encode(p, form) for p in pts])
        assert ok.all() and (out == want).all(), form
    assert {V.encode(p, 2)[0] for p in pts} == {2, 3} and {V.encode(p, 6)[0] for p in pts} == {6, 7}
    # every rejection, interleaved with keys that parse
    rej = V.key_rejections(valid_item[2]) + V.key_rejections(pts[0])
    keys = []
    for i, (_, k) in enumerate(rej):
        keys += [k, V.encode(pts[i % 64], (2, 6, 4)[i % 3])]
    out, ok = ctx.pubkey_parse_batch(keys)
    for i, (name, k) in enumerate(rej):
        assert ok[2 * i] == 0 and not out[2 * i].any(), name
        assert ok[2 * i + 1] == 1 and bytes(out[2 * i + 1]) == full[i % 64], name
        assert V.reencode(k) == (bytes(65), 0)
    for k in full[:8]:
        c = crypto.CompressPubkey(k, ctx)
        assert len(c) == 33 and c[0] == 2 | (k[64] & 1) and crypto.DecompressPubkey(c, ctx) == k
    with pytest.raises(crypto.ErrInvalidPubkey, match="invalid public key"):
        crypto.DecompressPubkey(b"\x02" + V.be32(M.P), ctx)
    with pytest.raises(crypto.ErrInvalidPubkey):
        crypto.CompressPubkey(b"\x04" + full[0][1:33] + V.be32(1), ctx)
