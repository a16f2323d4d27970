"""GPU parity of batched crypto.Sign (k_ecsign) and public-key derivation (k_pubkey_create) with the
reference's own signer: oracle.ref().gsvref_sign is secp256k1_ecdsa_sign_recoverable with
secp256k1_nonce_function_rfc6979, gsvref_pubkey is secp256k1_ec_pubkey_create.  Every comparison is
byte for byte.  The retry of the nonce counter cannot be reached by any input (tests/test_rfc6979_cpu.py
covers its nonce half on the CPU); recid 2 / 3 (R.x >= n) cannot be produced by any known nonce."""
import ctypes
import random

import numpy as np
import pytest

import rfc6979_model as M
from conftest import golden

pytestmark = pytest.mark.gpu
N = M.N
SHAPES = [1, 63, 64, 65, 255, 256, 257]
GUARD = 0xEE


def u8(b, width):
    return np.frombuffer(bytes(b), np.uint8).reshape(-1, width).copy()


def be32(x):
    return int(x).to_bytes(32, "big")


@pytest.fixture(scope="module")
def R(oracle):
    r = oracle.ref()
    assert r is not None, "the reference build oracle/_ref is needed (built by __graft_entry__.build())"
    return r


def ref_sign(R, key, msg):
    sig = ctypes.create_string_buffer(65)
    assert R.gsvref_sign(sig, msg, key) == 1
    return sig.raw


def ref_pub(R, key):
    pub = ctypes.create_string_buffer(65)
    assert R.gsvref_pubkey(pub, key) == 1
    return pub.raw


@pytest.fixture(scope="module")
def bulk(R):
    """4,096 seeded (key, msg) with the reference's signatures and keys, computed once"""
    pairs = M.random_pairs(4096, 0x516e)
    keys = u8(b"".join(k for k, _ in pairs), 32)
    msgs = u8(b"".join(m for _, m in pairs), 32)
    sigs = u8(b"".join(ref_sign(R, k, m) for k, m in pairs), 65)
    pubs = u8(b"".join(ref_pub(R, k) for k, _ in pairs), 65)
    for a in (keys, msgs, sigs, pubs):
        a.setflags(write=False)
    return keys, msgs, sigs, pubs


def dev_run(ctx, keys, msgs, want_addr=True, stream=None):
    """both _dev forms on one explicit stream, outputs over-allocated by a guard row:
    (sig, st, pub, addr, pst) with n + 1 rows each"""
    import torch
    dev = torch.device("cuda", ctx.device)
    n = keys.shape[0]
    d_key = torch.from_numpy(np.array(keys)).to(dev)
    d_msg = torch.from_numpy(np.array(msgs)).to(dev)
    outs = [torch.full(shape, GUARD, dtype=torch.uint8, device=dev)
            for shape in ((n + 1, 65), (n + 1,), (n + 1, 65), (n + 1, 20), (n + 1,))]
    d_sig, d_st, d_pub, d_addr, d_pst = outs
    torch.cuda.synchronize()
    cs = stream or torch.cuda.Stream()
    ctx.ecdsa_sign_batch_dev(d_msg, d_key, d_sig, d_st, stream=cs)
    ctx.pubkey_create_batch_dev(d_key, d_pub, d_addr if want_addr else None, d_pst, stream=cs)
    cs.synchronize()
    return [o.cpu().numpy() for o in outs]


# ---------------------------------------------------------------- 1. recorded rows
def test_golden_rows_host_and_dev(ctx, oracle):
    from gsv import crypto
    rows = golden("secp_sign.json")["rows"]
    keys = u8(b"".join(bytes.fromhex(r["key"]) for r in rows), 32)
    msgs = u8(b"".join(bytes.fromhex(r["msg"]) for r in rows), 32)
    want_sig = u8(b"".join(bytes.fromhex(r["sig"]) for r in rows), 65)
    want_pub = u8(b"".join(bytes.fromhex(r["pub"]) for r in rows), 65)
    sig, st = ctx.ecdsa_sign_batch(msgs, keys)
    assert (st == 0).all() and (sig == want_sig).all(), np.nonzero((sig != want_sig).any(axis=1))[0]
    pub, addr, pst = ctx.pubkey_create_batch(keys, want_addr=True)
    assert (pst == 0).all() and (pub == want_pub).all()
    for i in (0, 7, 63):
        assert bytes(addr[i]) == oracle.keccak256(bytes(want_pub[i, 1:]))[12:]
    n = len(rows)
    d_sig, d_st, d_pub, d_addr, d_pst = dev_run(ctx, keys, msgs)
    assert (d_sig[:n] == want_sig).all() and (d_st[:n] == 0).all()
    assert (d_pub[:n] == want_pub).all() and (d_addr[:n] == addr).all() and (d_pst[:n] == 0).all()
    # the crypto mirror, one item at a time
    r = rows[len(M.edge_pairs())]
    assert crypto.Sign(bytes.fromhex(r["msg"]), bytes.fromhex(r["key"]), ctx).hex() == r["sig"]
    assert crypto.Sign(bytes.fromhex(r["msg"]), int(r["key"], 16), ctx).hex() == r["sig"]
    assert crypto.PubkeyFromSeckey(int(r["key"], 16), ctx).hex() == r["pub"]
    assert crypto.Sign(bytes.fromhex(rows[0]["msg"]), b"\x01", ctx).hex() == rows[0]["sig"]  # key 1, padded
    for bad in (0, N, bytes(32)):
        with pytest.raises(crypto.ErrInvalidKey, match="invalid private key"):
            crypto.Sign(bytes(32), bad, ctx)
        with pytest.raises(crypto.ErrInvalidKey):
            crypto.PubkeyFromSeckey(bad, ctx)


# ---------------------------------------------------------------- 2. differential
def test_differential_4096(ctx, bulk):
    keys, msgs, want_sig, want_pub = bulk
    sig, st = ctx.ecdsa_sign_batch(msgs, keys)
    assert (st == 0).all()
    assert (sig == want_sig).all(), np.nonzero((sig != want_sig).any(axis=1))[0][:10]
    assert set(sig[:, 64]) == {0, 1}  # both recids present
    pub, _, pst = ctx.pubkey_create_batch(keys)
    assert (pst == 0).all() and (pub == want_pub).all()
    # the same signatures recover those keys, and verify against them
    rpub, _, rst = ctx.ecrecover_batch(msgs, sig, want_pub=True, want_addr=False)
    assert (rst == 0).all() and (rpub == pub).all()
    ok = ctx.ecdsa_verify_batch(msgs, sig[:, :64], [bytes(p) for p in pub])
    assert (ok == 1).all()


# ---------------------------------------------------------------- 3. launch-shape edges
def test_empty_batch(ctx):
    from gsv import _lib
    L = _lib.load()
    sig, st = ctx.ecdsa_sign_batch(np.zeros((0, 32), np.uint8), np.zeros((0, 32), np.uint8))
    assert sig.shape == (0, 65) and st.shape == (0,)
    pub, addr, pst = ctx.pubkey_create_batch(np.zeros((0, 32), np.uint8), want_addr=True)
    assert pub.shape == (0, 65) and addr.shape == (0, 20) and pst.shape == (0,)
    assert L.gsv_ecdsa_sign_batch(ctx.handle, None, None, 0, None, None) == 0
    assert L.gsv_ecdsa_sign_batch_dev(ctx.handle, None, None, 0, None, None, None) == 0
    assert L.gsv_pubkey_create_batch(ctx.handle, None, 0, None, None, None) == 0
    assert L.gsv_pubkey_create_batch_dev(ctx.handle, None, 0, None, None, None, None) == 0
    # n = 0 through the _dev forms writes nothing
    d_sig, d_st, d_pub, d_addr, d_pst = dev_run(ctx, np.zeros((0, 32), np.uint8), np.zeros((0, 32), np.uint8))
    for o in (d_sig, d_st, d_pub, d_addr, d_pst):
        assert (o == GUARD).all()
    # argument errors, not faults
    b = np.zeros(65, np.uint8)
    p = b.ctypes.data
    E = _lib.E_INVALID_ARG
    assert L.gsv_ecdsa_sign_batch(ctx.handle, None, p, 1, p, p) == E
    assert L.gsv_ecdsa_sign_batch(ctx.handle, p, None, 1, p, p) == E
    assert L.gsv_ecdsa_sign_batch(ctx.handle, p, p, 1, None, p) == E
    assert L.gsv_ecdsa_sign_batch(ctx.handle, p, p, 1, p, None) == E
    assert L.gsv_ecdsa_sign_batch(ctx.handle, p, p, 1 << 32, p, p) == E
    assert L.gsv_pubkey_create_batch(ctx.handle, None, 1, p, None, p) == E
    assert L.gsv_pubkey_create_batch(ctx.handle, p, 1, None, None, p) == E
    assert L.gsv_pubkey_create_batch(ctx.handle, p, 1, p, None, None) == E


@pytest.mark.parametrize("n", SHAPES)
def test_launch_shapes(ctx, bulk, n):
    keys, msgs, want_sig, want_pub = (a[:n] for a in bulk)
    d_sig, d_st, d_pub, d_addr, d_pst = dev_run(ctx, keys, msgs)
    # the last item against the reference, then all of them; the guard row behind each output untouched
    assert bytes(d_sig[n - 1]) == bytes(want_sig[n - 1]) and bytes(d_pub[n - 1]) == bytes(want_pub[n - 1])
    assert (d_sig[:n] == want_sig).all() and (d_pub[:n] == want_pub).all()
    assert (d_st[:n] == 0).all() and (d_pst[:n] == 0).all()
    for o in (d_sig, d_st, d_pub, d_addr, d_pst):
        assert (o[n:] == GUARD).all()
    sig, st = ctx.ecdsa_sign_batch(msgs, keys)
    pub, addr, pst = ctx.pubkey_create_batch(keys, want_addr=True)
    assert (sig == want_sig).all() and (pub == want_pub).all() and (addr == d_addr[:n]).all()
    # without the address output nothing is written there
    assert (dev_run(ctx, keys, msgs, want_addr=False)[3] == GUARD).all()


# ---------------------------------------------------------------- 4. the key rule
def test_key_rule(ctx, R, bulk):
    from gsv import _lib
    keys, msgs, want_sig, want_pub = (a[:64 * 6].copy() for a in bulk)
    special = [0, N, N + 1, 2**256 - 1, 1, N - 1]
    bad = [True, True, True, True, False, False]
    where = [64 * i + i % 64 for i in range(len(special))]  # each in a wave of its own, among 63 ordinary lanes
    for w, k in zip(where, special):
        keys[w] = np.frombuffer(be32(k), np.uint8)
    for via in ("host", "dev"):
        if via == "host":
            sig, st = ctx.ecdsa_sign_batch(msgs, keys)
            pub, addr, pst = ctx.pubkey_create_batch(keys, want_addr=True)
        else:
            sig, st, pub, addr, pst = (o[:len(keys)] for o in dev_run(ctx, keys, msgs))
        rest = np.ones(len(keys), bool)
        rest[where] = False
        assert (st[rest] == 0).all() and (sig[rest] == want_sig[rest]).all(), via
        assert (pst[rest] == 0).all() and (pub[rest] == want_pub[rest]).all(), via
        for w, k, b in zip(where, special, bad):
            if b:
                assert st[w] == pst[w] == _lib.ST_INVALID_KEY == 11, (via, hex(k))
                assert not sig[w].any() and not pub[w].any() and not addr[w].any(), (via, hex(k))
            else:
                assert st[w] == pst[w] == 0, (via, hex(k))
                assert bytes(sig[w]) == ref_sign(R, be32(k), bytes(msgs[w])), (via, hex(k))
                assert bytes(pub[w]) == ref_pub(R, be32(k)), (via, hex(k))
    # a batch of bad keys alone: whole waves of them
    z, zst = ctx.ecdsa_sign_batch(msgs[:65], np.zeros((65, 32), np.uint8))
    assert (zst == 11).all() and not z.any()


# ---------------------------------------------------------------- 5. message edges
def test_message_edges(ctx, R):
    ms = [0, N - 1, N, N + 1, 2**256 - 1]
    ks = [1, N - 1, 0x1234567890abcdef << 64]
    pairs = [(be32(k), be32(m)) for k in ks for m in ms]
    sig, st = ctx.ecdsa_sign_batch(u8(b"".join(m for _, m in pairs), 32), u8(b"".join(k for k, _ in pairs), 32))
    assert (st == 0).all()
    for (k, m), s in zip(pairs, sig):
        assert bytes(s) == ref_sign(R, k, m), (k.hex(), m.hex())
    # the raw bytes feed the nonce and the reduced value feeds s: msg = n and msg = 0 sign differently
    for i in range(len(ks)):
        assert bytes(sig[5 * i]) != bytes(sig[5 * i + 2])


# ---------------------------------------------------------------- 6. secret hygiene
def test_staged_keys_are_wiped(ctx):
    """after the host forms return, the arena's key region (the first region: offset 0, 32 n bytes,
    tests/test_sign_stage_host.py) holds none of the key bytes; the region behind it still holds the
    messages, so the read looks at the arena this call staged in"""
    n = 300
    keys = np.full((n, 32), 0xA5, np.uint8)
    msgs = np.full((n, 32), 0x3C, np.uint8)
    sig, st = ctx.ecdsa_sign_batch(msgs, keys)
    assert (st == 0).all() and sig.any()
    region = ctx._arena_read(0, n * 32)
    assert not region.any(), "staged secret keys left in the arena"
    behind = (n * 32 + 255) // 256 * 256
    assert (ctx._arena_read(behind, n * 32) == 0x3C).all()
    pub, _, pst = ctx.pubkey_create_batch(keys)
    assert (pst == 0).all() and pub.any()
    assert not ctx._arena_read(0, n * 32).any()


# ---------------------------------------------------------------- 7. capture
def test_dev_form_is_capturable(ctx, bulk):
    import torch
    from gsv import _lib
    dev = torch.device("cuda", ctx.device)
    n = 257
    keys, msgs, want_sig, want_pub = (a[:n] for a in bulk)
    d_key = torch.from_numpy(np.array(keys)).to(dev)
    d_msg = torch.from_numpy(np.array(msgs)).to(dev)
    d_sig = torch.full((n, 65), GUARD, dtype=torch.uint8, device=dev)
    d_st = torch.full((n,), GUARD, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    cs = torch.cuda.Stream()
    # one launch per call, timed under K_ECRECOVER
    ctx.set_timing(True)
    try:
        ctx.reset_timing()
        ctx.ecdsa_sign_batch_dev(d_msg, d_key, d_sig, d_st, stream=cs)
        cs.synchronize()
        ms, launches = ctx.kernel_time(_lib.K_ECRECOVER)
        assert launches == 1 and ms > 0
    finally:
        ctx.set_timing(False)
        ctx.reset_timing()
    assert (d_sig.cpu().numpy() == want_sig).all()
    # captured on an explicit stream (nothing allocated, nothing synchronised inside), replayed twice
    g = torch.cuda.CUDAGraph()
    shapes_before = ctx.prepared_shapes()
    with torch.cuda.graph(g, stream=cs):
        ctx.ecdsa_sign_batch_dev(d_msg, d_key, d_sig, d_st, stream=cs)
    assert ctx.prepared_shapes() == shapes_before
    for _ in range(2):
        d_sig.fill_(GUARD)
        d_st.fill_(GUARD)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert (d_sig.cpu().numpy() == want_sig).all() and (d_st.cpu().numpy() == 0).all()


# ---------------------------------------------------------------- 8. headers
def test_sign_headers_then_verify(ctx):
    from gsv import _lib, crypto, sharding
    rng = random.Random(0x4ead)
    n = 64
    keys = [rng.randrange(1, N) for _ in range(n)]
    _, addr, st = ctx.pubkey_create_batch(u8(b"".join(be32(k) for k in keys), 32), want_addr=True)
    assert (st == 0).all()

    def headers():
        return [sharding.CollationHeader(i, bytes(rng.getrandbits(8) for _ in range(32)), 1000 + i, bytes(addr[i]))
                for i in range(n)]

    hs = headers()
    sharding.SignHeaders(hs, keys, ctx)
    assert all(h.Sig() is not None and len(h.Sig()) == 65 and h.Sig()[64] in (0, 1) for h in hs)
    signer, vst = sharding.VerifyProposerSignatures(hs, ctx)
    assert (vst == _lib.ST_OK).all() and (signer == addr).all()
    # one header signed with another header's key
    hs = headers()
    swapped = list(keys)
    swapped[5] = keys[6]
    sharding.SignHeaders(hs, swapped, ctx)
    _, vst = sharding.VerifyProposerSignatures(hs, ctx)
    assert vst[5] == _lib.ST_PROPOSER_MISMATCH and (np.delete(vst, 5) == _lib.ST_OK).all()
    # a bad key raises and leaves every header untouched
    hs = headers()
    for bad in (0, N, 1 << 256):
        with pytest.raises(crypto.ErrInvalidKey):
            sharding.SignHeaders(hs, keys[:9] + [bad] + keys[10:], ctx)
        assert all(h.Sig() is None for h in hs)


# ---------------------------------------------------------------- 9. the synthetic signer is unchanged
def test_synth_sign_unchanged(ctx, R):
    """ecdsa_sign was split for k_ecsign: k_synth_sign's 4,096 items still equal the reference's signer
    run with the generator's keys and nonces"""
    n, seed = 4096, 20241
    u8p = ctypes.POINTER(ctypes.c_uint8)
    R.gsvref_synth_sign_many.argtypes = [ctypes.c_uint64, ctypes.c_long, ctypes.c_long, u8p, u8p]
    R.gsvref_synth_sign_many.restype = ctypes.c_long
    wmsg, wsig = np.zeros((n, 32), np.uint8), np.zeros((n, 65), np.uint8)
    assert R.gsvref_synth_sign_many(seed, 0, n, wmsg.ctypes.data_as(u8p), wsig.ctypes.data_as(u8p)) == n
    msg, sig, pub, addr = ctx.synth_sign(seed=seed, n=n)
    assert (msg == wmsg).all() and (sig == wsig).all()
    rpub, raddr, st = ctx.ecrecover_batch(msg, sig, want_pub=True, want_addr=True)
    assert (st == 0).all() and (rpub == pub).all() and (raddr == addr).all()
