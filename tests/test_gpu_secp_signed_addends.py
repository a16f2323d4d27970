"""GPU parity of the recovery with its subtractions inside the products (secp256k1_fe9.cuh: fe9_mul_sub,
fe9_sqr_sub2 in the mixed adds, the doubling, the table's co-Z steps and the twisted tail): keys,
addresses and statuses bit for bit against the oracle through the four kernels that inline recover_core
(k_ecrecover, k_sender, the ecrecover precompile, the notary's transaction kernel), on three batches:

  * 1,024 random signatures: four blocks, so both the LDS and the private half of the GLV table and both
    signs of the digits occur in every wave;
  * the crafted exceptional scalars of tests/secp_glv_model.py: u2 = -26 lambda (the ladder's one
    doubling) alone and mixed into a wave of ordinary items, every other exceptional scalar, and u1 = 0;
  * the edges: r, s in {0, 1, n - 1, n}, recid 2 / 3 around r = p - n (r + n must stay below p), and an r
    that is no x-coordinate."""
import ctypes
import random

import numpy as np
import pytest

import secp_glv_model as M
from test_gpu_secp256k1_scalars import U2_DOUBLING, _be32, _crafted_tx, _pack, _pub65, _random_point

pytestmark = pytest.mark.gpu
N, P = M.N, M.P


# ---------------------------------------------------------------- the four paths against the oracle
def _plain(oracle, msgs, sigs, homestead):
    L = oracle.lib()
    n = msgs.shape[0]
    st, addr = np.zeros(n, np.uint8), np.zeros((n, 20), np.uint8)
    for i in range(n):
        buf = ctypes.create_string_buffer(20)
        st[i] = L.oracle_recover_plain(buf, bytes(msgs[i]), bytes(sigs[i, :32]), 32, bytes(sigs[i, 32:64]), 32,
                                       bytes([27 + sigs[i, 64]]), 1, homestead)
        if st[i] == 0:
            addr[i] = np.frombuffer(buf.raw, np.uint8)
    return st, addr


def _check_recover_sender_precompile(ctx, oracle, msgs, sigs):
    """returns the oracle's ecrecover statuses"""
    n = msgs.shape[0]
    pub, addr, st = ctx.ecrecover_batch(msgs, sigs, want_pub=True, want_addr=True)
    opub, ost = oracle.ecrecover_batch(msgs, sigs, threads=16)
    assert (st == ost).all(), np.nonzero(st != ost)[0][:10]
    assert (pub == opub).all(), np.nonzero((pub != opub).any(axis=1))[0][:10]
    for i in np.nonzero(ost == 0)[0]:
        assert bytes(addr[i]) == oracle.keccak256(bytes(opub[i, 1:]))[12:], i
    V = sigs[:, 64].astype(np.uint64) + 27
    plain = {}
    for homestead in (0, 1):
        want_st, want_addr = plain[homestead] = _plain(oracle, msgs, sigs, homestead)
        a, s = ctx.sender_batch(msgs, sigs[:, :32], sigs[:, 32:64], V, np.zeros(n, np.uint8), bool(homestead))
        assert (s == want_st).all(), (homestead, np.nonzero(s != want_st)[0][:10])
        assert (a[s == 0] == want_addr[s == 0]).all(), homestead
    want_st, want_addr = plain[0]
    inputs = [bytes(msgs[i]) + bytes(31) + bytes([27 + sigs[i, 64]]) + bytes(sigs[i, :64]) for i in range(n)]
    out, ok = ctx.ecrecover_precompile_batch(inputs)
    assert ((ok == 1) == (want_st == 0)).all(), np.nonzero((ok == 1) != (want_st == 0))[0][:10]
    assert not out[:, :12].any() and (out[want_st == 0, 12:] == want_addr[want_st == 0]).all()
    assert not out[want_st != 0].any()
    return ost


def _check_notary(ctx, oracle, txs, chain_id, signer=0):
    """the notary's transaction kernel and tx_sender_batch against the oracle's sender; returns the statuses"""
    want = [oracle.tx_sender(t, chain_id, signer) for t in txs]
    max_txs = (len(txs) + 7) // 8 * 8
    _, ntx, bitmap, senders, status = ctx.notary_validate_shards([oracle.blob_serialize(txs)], chain_id, signer, max_txs)
    addr, st = ctx.tx_sender_batch(txs, chain_id, signer)
    assert ntx[0] == len(txs)
    for t, (s, a) in enumerate(want):
        assert status[0, t] == s and st[t] == s, (t, status[0, t], st[t], s)
        assert ((bitmap[0, t // 8] >> (t % 8)) & 1) == (s == 0), t
        if s == 0:
            assert bytes(senders[0, t]) == a and bytes(addr[t]) == a, t
    return [s for s, _ in want]


# ---------------------------------------------------------------- 1. random, four blocks
def test_random_batch_of_four_blocks(ctx, oracle):
    msgs, sigs, _, _ = ctx.synth_sign(seed=909, n=1024, want_pub=False, want_addr=False)
    ost = _check_recover_sender_precompile(ctx, oracle, msgs, sigs)
    assert (ost == 0).all()


def test_random_batch_through_the_notary(ctx, oracle):
    rng = random.Random(0x909)
    txs = [_crafted_tx(oracle, rng, i, rng.randrange(1, N), 1 if i % 2 else None) for i in range(1024)]
    assert all(s == 0 for s in _check_notary(ctx, oracle, txs, 1))


# ---------------------------------------------------------------- 2. the exceptional scalars
@pytest.fixture(scope="module")
def exceptional():
    exc = M.exceptional_scalars()
    assert U2_DOUBLING in exc
    return [U2_DOUBLING] + sorted(u for u in exc if u != U2_DOUBLING)


def test_exceptional_scalars(ctx, oracle, exceptional):
    rng = random.Random(0xe5c)
    lone = [(_random_point(rng), rng.randrange(1, N), U2_DOUBLING)]
    # a wave of ordinary items with the doubling at lanes 0, 31 and 63, one of them with u1 = 0
    wave = [(_random_point(rng), rng.randrange(1, N), rng.randrange(1, N)) for _ in range(64)]
    for lane, u1 in ((0, rng.randrange(1, N)), (31, 0), (63, 1)):
        wave[lane] = (wave[lane][0], u1, U2_DOUBLING)
    # every exceptional scalar with u1 random and u1 = 0, then ordinary u2 with u1 = 0
    rest = [(_random_point(rng), u1, u2) for u2 in exceptional for u1 in (rng.randrange(1, N), 0)]
    rest += [(_random_point(rng), 0, rng.randrange(1, N)) for _ in range(8)]
    for items in (lone, wave, rest):
        msgs, sigs = _pack(items)
        ost = _check_recover_sender_precompile(ctx, oracle, msgs, sigs)
        assert (ost == 0).all()
        pub, _, _ = ctx.ecrecover_batch(msgs, sigs, want_pub=True, want_addr=False)
        for i, it in enumerate(items):  # Python integers as well
            if it[2] in exceptional or it[1] == 0:
                assert (pub[i] == _pub65(M.recover_expected(*it))).all(), i


def test_exceptional_scalars_through_the_notary(ctx, oracle, exceptional):
    rng = random.Random(0xe5d)
    lone = [_crafted_tx(oracle, rng, 0, U2_DOUBLING, 1)]
    wave = [_crafted_tx(oracle, rng, i, U2_DOUBLING if i in (0, 31, 63) else rng.randrange(1, N), 1 if i % 2 else None)
            for i in range(64)]
    rest = [_crafted_tx(oracle, rng, i, u2, 1 if i % 2 else None) for i, u2 in enumerate(exceptional)]
    for txs in (lone, wave, rest):
        assert all(s == 0 for s in _check_notary(ctx, oracle, txs, 1))


# ---------------------------------------------------------------- 3. the edges
def _non_residue_x(rng):
    while True:
        x = rng.randrange(1, N)
        if M.lift_x(x, 0) is None:
            return x


def _edge_rs():
    rng = random.Random(0xed9e)
    edge = (0, 1, N - 1, N)
    rs = [(r, s) for r in edge for s in edge]
    rs += [(r, rng.randrange(1, N)) for r in edge] + [(rng.randrange(1, N), s) for s in edge]
    rs += [(_non_residue_x(rng), rng.randrange(1, N)) for _ in range(4)]
    # r + n against p (recids 2 and 3 read x = r + n): below, at and above p - n, and small r
    rs += [(r, rng.randrange(1, N)) for r in (P - N - 2, P - N - 1, P - N, P - N + 1, 1, 2, 3, 4, 5, 6, 7, 8)]
    return rs


def test_edge_batch(ctx, oracle):
    rng = random.Random(0xed9f)
    rows = [(r, s, recid) for (r, s) in _edge_rs() for recid in (0, 1, 2, 3)]
    msgs = np.array([np.frombuffer(bytes(rng.getrandbits(8) for _ in range(32)), np.uint8) for _ in rows])
    sigs = np.array([np.frombuffer(_be32(r) + _be32(s) + bytes([recid]), np.uint8) for r, s, recid in rows])
    ost = _check_recover_sender_precompile(ctx, oracle, msgs, sigs)
    st = dict(zip(rows, ost.tolist()))
    assert all(st[(r, s, k)] != 0 for (r, s, k) in rows if r in (0, N) or s in (0, N))
    assert all(st[(r, s, k)] != 0 for (r, s, k) in rows if k >= 2 and r >= P - N)
    assert any(v == 0 for (r, s, k), v in st.items() if k >= 2) and any(v == 0 for (r, s, k), v in st.items() if k < 2)


def test_edge_batch_through_the_notary(ctx, oracle):
    rng = random.Random(0xeda0)
    txs = []
    for i, (r, s) in enumerate(_edge_rs()):
        for parity in (0, 1):
            fields = (oracle.rlp_uint(i) + oracle.rlp_uint(20 * 10 ** 9) + oracle.rlp_uint(21000) +
                      oracle.rlp_string(bytes(range(1, 21))) + oracle.rlp_uint(10 ** 18 + i) + oracle.rlp_string(b""))
            v = parity + (27 if i % 2 else 37)
            txs.append(oracle.rlp_list(fields + oracle.rlp_uint(v) + oracle.rlp_uint(r) + oracle.rlp_uint(s)))
    for signer in (0, 2):  # EIP155Signer(1) and FrontierSigner (high s admitted)
        got = _check_notary(ctx, oracle, txs, 1, signer)
        assert any(s == 0 for s in got) and any(s != 0 for s in got)
