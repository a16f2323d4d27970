"""GPU parity of the four kernels that inline recover_core (k_ecrecover, k_sender, the ecrecover
precompile, k_notary_tx) after the GLV ladder and the comb moved to the W convention ((X, 2Y, Z)
accumulators, a doubling that returns -2P: secp256k1_fe9.cuh gejw_*), bit-exact against the oracle:

  * batches of 1, 63, 64, 65, 257 and 4,096 ordinary signatures (a lone lane, a wave less one, a full
    wave, one lane into the next wave, one lane into the next block, many blocks);
  * chosen scalars (tests/secp_glv_model.py craft): u2 = -26 lambda, the one scalar that reaches the
    out-of-line doubling (now gejw_dbl: +2P with W at magnitude 2), u2 in {1, 2, 3, n - 1, lambda,
    n - lambda}, u1 = 0, all four recids, and one item of every failure class.

Results only.  The CPU side of the same change: tests/test_fe9_wconv.py, tests/test_asm_emulated_wconv.py."""
import random

import numpy as np
import pytest

import secp_glv_model as M
import test_gpu_secp256k1_scalars as S

pytestmark = pytest.mark.gpu
N, P, LAM = M.N, M.P, M.LAMBDA
ST_OK = 0
SIZES = (1, 63, 64, 65, 257, 4096)
U2S = (S.U2_DOUBLING, 1, 2, 3, N - 1, LAM, N - LAM)


@pytest.fixture(scope="module")
def signed(ctx, oracle):
    """4,096 synthetic signatures and the oracle's keys and addresses for them (computed once)"""
    msg, sig, _, _ = ctx.synth_sign(seed=7070, n=max(SIZES), want_pub=False, want_addr=False)
    opub, ost = oracle.ecrecover_batch(msg, sig, threads=16)
    assert (ost == ST_OK).all()
    return msg, sig, opub, S._addresses(oracle, opub)


@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes_ecrecover_sender_precompile(ctx, signed, n):
    msg, sig, opub, oaddr = (a[:n] for a in signed)
    pub, addr, st = ctx.ecrecover_batch(msg, sig, want_pub=True, want_addr=True)
    assert (st == ST_OK).all() and (pub == opub).all() and (addr == oaddr).all()
    V = sig[:, 64].astype(np.uint64) + 27
    addr, st = ctx.sender_batch(msg, sig[:, :32], sig[:, 32:64], V, np.zeros(n, np.uint8), True)
    assert (st == ST_OK).all() and (addr == oaddr).all()
    inputs = [bytes(msg[i]) + bytes(31) + bytes([27 + sig[i, 64]]) + bytes(sig[i, :64]) for i in range(n)]
    out, ok = ctx.ecrecover_precompile_batch(inputs)
    assert ok.all() and not out[:, :12].any() and (out[:, 12:] == oaddr).all()


def test_batch_sizes_notary(ctx, oracle):
    """one shard per batch size; every transaction signed by a chosen (r, s) (random u2), half EIP-155"""
    rng = random.Random(0x3a7)
    chain_id = 1
    shards = []
    for n in SIZES:
        shards.append([S._crafted_tx(oracle, rng, i, rng.randrange(1, N), chain_id if i % 2 else None)
                       for i in range(n)])
    bodies = [oracle.blob_serialize(txs) for txs in shards]
    _, ntx, bitmap, senders, status = ctx.notary_validate_shards(bodies, chain_id, 0, max(SIZES))
    for k, txs in enumerate(shards):
        assert ntx[k] == len(txs)
        for t, tx in enumerate(txs):
            s, a = oracle.tx_sender(tx, chain_id, 0)
            assert s == ST_OK and status[k, t] == s, (k, t, status[k, t])
            assert (bitmap[k, t // 8] >> (t % 8)) & 1
            assert bytes(senders[k, t]) == a, (k, t)


def _high_x_points():
    """curve points with n <= x < p, both parities: signatures with recid 2 and 3 (r = x - n)"""
    out = []
    k = 1
    while len(out) < 2:
        R = M.lift_x(N + k, 0)
        if R is not None:
            out.append((k, R))
        k += 1
    return [(k, (R[0], y)) for k, R in out for y in (R[1], P - R[1])]


@pytest.fixture(scope="module")
def chosen():
    """(msgs, sigs, want): the chosen scalars on points of both parities with u1 random, 0 and 1 (recid 0, 1),
    then on points with x >= n (recid 2, 3); want = u1 G + u2 R by Python integers"""
    rng = random.Random(0x2b0c)
    items = []
    for u2 in U2S:
        for _ in range(2):
            R = S._random_point(rng)
            for Rp in (R, (R[0], P - R[1])):
                for u1 in (rng.randrange(1, N), 0, 1):
                    items.append((Rp, u1, u2))
    msgs, sigs = S._pack(items)
    want = [M.recover_expected(*it) for it in items]
    hm, hs = [], []
    for k, R in _high_x_points():
        for u2 in U2S:
            for u1 in (rng.randrange(1, N), 0):
                hm.append(S._be32((-u1 * k) % N))
                hs.append(S._be32(k) + S._be32(u2 * k % N) + bytes([2 | (R[1] & 1)]))
                want.append(M.recover_expected(R, u1, u2))
    msgs = np.concatenate([msgs, np.frombuffer(b"".join(hm), np.uint8).reshape(-1, 32)])
    sigs = np.concatenate([sigs, np.frombuffer(b"".join(hs), np.uint8).reshape(-1, 65)])
    assert set(sigs[:, 64]) == {0, 1, 2, 3} and all(w is not None for w in want)
    return msgs, sigs, np.array([S._pub65(w) for w in want])


def test_chosen_scalars_ecrecover(ctx, oracle, chosen):
    msgs, sigs, want = chosen
    pub, addr, st = ctx.ecrecover_batch(msgs, sigs, want_pub=True, want_addr=True)
    S._check_against_oracle(oracle, msgs, sigs, pub, addr, st)
    assert (pub == want).all()
    # the out-of-line doubling alone in its wave (a batch of one)
    p1, _, s1 = ctx.ecrecover_batch(msgs[:1], sigs[:1], want_pub=True, want_addr=False)
    assert s1[0] == ST_OK and (p1[0] == want[0]).all()


def test_chosen_scalars_sender_and_precompile(ctx, oracle, chosen):
    msgs, sigs, want = chosen
    low = sigs[:, 64] < 2  # V = 27 + recid: the plain paths take recid 0 and 1
    msgs, sigs, waddr = msgs[low], sigs[low], S._addresses(oracle, want[low])
    V = sigs[:, 64].astype(np.uint64) + 27
    addr, st = ctx.sender_batch(msgs, sigs[:, :32], sigs[:, 32:64], V, np.zeros(len(V), np.uint8), False)
    assert (st == ST_OK).all() and (addr == waddr).all()
    inputs = [bytes(msgs[i]) + bytes(31) + bytes([27 + sigs[i, 64]]) + bytes(sigs[i, :64]) for i in range(len(msgs))]
    out, ok = ctx.ecrecover_precompile_batch(inputs)
    assert ok.all() and not out[:, :12].any() and (out[:, 12:] == waddr).all()


def test_chosen_scalars_notary(ctx, oracle):
    rng = random.Random(0x91)
    chain_id = 1
    txs = []
    for i, u2 in enumerate(U2S):
        txs.append(S._crafted_tx(oracle, rng, 2 * i, u2, chain_id))
        txs.append(S._crafted_tx(oracle, rng, 2 * i + 1, u2, None))
    body = oracle.blob_serialize(txs)
    _, ntx, bitmap, senders, status = ctx.notary_validate_shards([body], chain_id, 0, 64)
    addr, st = ctx.tx_sender_batch(txs, chain_id, 0)
    assert ntx[0] == len(txs)
    for t, tx in enumerate(txs):
        s, a = oracle.tx_sender(tx, chain_id, 0)
        assert s == ST_OK and status[0, t] == s and st[t] == s, (t, status[0, t], st[t])
        assert bytes(senders[0, t]) == a and bytes(addr[t]) == a, t


def test_failure_classes(ctx, oracle):
    """one item of every way recover_core refuses: r = 0, s = 0, r >= n, s >= n, recid & 2 with
    r >= p - n, recid > 3, x_R not on the curve, and u1 G + u2 R = O — status and key as the oracle's"""
    rng = random.Random(0xfa11)
    k = rng.randrange(1, N)
    R = M.ec_mul(k, M.G)
    while R[0] >= N:
        k += 1
        R = M.ec_mul(k, M.G)
    u2 = rng.randrange(1, N)
    good = M.craft(R, rng.randrange(1, N), u2)
    x_off = next(x for x in range(2, 100) if M.lift_x(x, 0) is None)
    rows = [
        (good[0], 0, good[2], good[3]),
        (good[0], good[1], 0, good[3]),
        (good[0], N, good[2], good[3]),
        (good[0], good[1], N + 1, good[3]),
        (good[0], P - N, good[2], 2),
        (good[0], good[1], good[2], 4),
        (good[0], x_off, u2 * x_off % N, 0),
        M.craft(R, (-u2 * k) % N, u2),  # u1 G = -u2 R: the sum is the identity
        good,
    ]
    msgs = np.array([np.frombuffer(S._be32(m), np.uint8) for m, _, _, _ in rows])
    sigs = np.array([np.frombuffer(S._be32(r) + S._be32(s) + bytes([v]), np.uint8) for _, r, s, v in rows])
    opub, ost = oracle.ecrecover_batch(msgs, sigs)
    assert (ost[:-1] != ST_OK).all() and ost[-1] == ST_OK
    pub, _, st = ctx.ecrecover_batch(msgs, sigs, want_pub=True, want_addr=False)
    assert (st == ost).all(), (st, ost)
    assert (pub == opub).all()
