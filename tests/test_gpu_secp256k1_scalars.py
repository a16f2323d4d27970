"""GPU parity of secp256k1 recovery on chosen scalars.  recover_core (recover_dev.cuh) computes
u1 G + u2 R with u1 = -m/r, u2 = s/r; ordinary signatures make both uniform random.  Here they are chosen:
for a curve point R = (x, y) with x < n, sig = (r = x, s = u2 r, recid = y & 1) and msg = -u1 r recover
u1 G + u2 R (tests/secp_glv_model.py craft; checked against the oracle and Python integers on the CPU in
tests/test_secp_glv_cpu.py).

  * the scalars whose GLV ladder meets an exceptional mixed add (the model's list: the out-of-line doubling
    gej9_dbl_rare is reached by no other input), alone in a wave and among ordinary lanes;
  * small and near-lattice u2 (a + b lambda, and the neighbourhoods of n, n/2, 2^128, 2^129, +-lambda, the
    lattice vectors and t n/M), with u1 at the comb's edges;
  * the same inputs through the sender, precompile and notary kernels, which inline recover_core;
  * every reachable entry of the fixed-base comb table: u1 = d 2^(COMB_BITS w) for all d, window by window.

Expected keys come from the oracle for every item (bit-exact status, key, address), from affine Python
integers for every special and a seeded sample; the comb sweep's keys are tied together by the oracle's
inversion-free chain check (Q[d] = Q[d-1] + 2^(COMB_BITS w) G) and anchored to the oracle at sampled d."""
import ctypes
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import secp_glv_model as M

pytestmark = pytest.mark.gpu
N, LAM = M.N, M.LAMBDA
ST_OK, ST_INVALID_SIG = 0, 5
U2_DOUBLING = (-26 * LAM) % N  # split (0, -26), v1 branch: the last lambda add finds acc == P


def _be32(v):
    return int(v).to_bytes(32, "big")


def _random_point(rng, want_low_s_for=None):
    """a curve point with x < n and random y parity (x u2 <= n/2 when a scalar is given: a low s)"""
    while True:
        x = rng.randrange(1, N)
        R = M.lift_x(x, rng.randrange(2))
        if R is not None and (want_low_s_for is None or x * want_low_s_for % N <= M.HALF_N):
            return R


def _pack(items):
    """[(R, u1, u2)] -> msgs (n, 32), sigs (n, 65)"""
    msgs = np.zeros((len(items), 32), np.uint8)
    sigs = np.zeros((len(items), 65), np.uint8)
    for i, (R, u1, u2) in enumerate(items):
        msg, r, s, recid = M.craft(R, u1, u2)
        msgs[i] = np.frombuffer(_be32(msg), np.uint8)
        sigs[i] = np.frombuffer(_be32(r) + _be32(s) + bytes([recid]), np.uint8)
    return msgs, sigs


def _pub65(q):
    return np.frombuffer(b"\x04" + _be32(q[0]) + _be32(q[1]), np.uint8)


def _addresses(oracle, pub):
    return np.array([np.frombuffer(oracle.keccak256(bytes(p[1:]))[12:], np.uint8) for p in pub])


def _check_against_oracle(oracle, msgs, sigs, pub, addr, st):
    """status, key and address of every item against the oracle, bit for bit"""
    opub, ost = oracle.ecrecover_batch(msgs, sigs, threads=16)
    assert (ost == ST_OK).all(), np.nonzero(ost != ST_OK)[0][:10]  # no crafted item is refused by the reference
    assert (st == ost).all(), np.nonzero(st != ost)[0][:10]
    assert (pub == opub).all(), np.nonzero((pub != opub).any(axis=1))[0][:10]
    assert (addr == _addresses(oracle, opub)).all()


# ---------------------------------------------------------------- the crafted sets (built once)
@pytest.fixture(scope="module")
def exceptional():
    """the scalars whose ladder meets an exceptional add, per the model; the doubling first"""
    exc = M.exceptional_scalars()
    assert U2_DOUBLING in exc and ("dbl", 0, 1) in exc[U2_DOUBLING]
    return [U2_DOUBLING] + sorted(u for u in exc if u != U2_DOUBLING)


@pytest.fixture(scope="module")
def specials(exceptional):
    """every exceptional u2 with four points R, both parities of y_R each, and u1 random, 0 and 1"""
    rng = random.Random(0x5ec9)
    items = []
    for u2 in exceptional:
        for _ in range(4):
            R = _random_point(rng)
            for Rp in (R, (R[0], M.P - R[1])):
                for u1 in (rng.randrange(1, N), 0, 1):
                    items.append((Rp, u1, u2))
    return items


def _u1_rotation(rng, i):
    w = 1 + (i // 7) % (M.COMB_WINDOWS - 1)
    top = M.COMB_BITS * (M.COMB_WINDOWS - 1)
    return (rng.randrange(1, N), 0, 1, N - 1, 1 << (M.COMB_BITS * w), (1 << (M.COMB_BITS * w)) - 1,
            ((N - 1) >> top) << top)[i % 7]


@pytest.fixture(scope="module")
def families():
    """(items, n_small): a + b lambda for |a|, |b| <= 40, then the near-constant family; R from a pool of
    16 points, u1 rotating through random, 0, 1, n - 1, 2^(20w), 2^(20w) - 1 and the largest d 2^240 < n"""
    rng = random.Random(0xfa31)
    pool = [_random_point(rng) for _ in range(16)]
    small = [u for u, _, _ in M.small_family(40)]
    assert len(small) == 6560
    scalars = small + M.family("near")
    return [(pool[i % 16], _u1_rotation(rng, i), u2) for i, u2 in enumerate(scalars)], len(small)


@pytest.fixture(scope="module")
def crafted(specials, families):
    """the specials and both families as one batch: (items, msgs, sigs)"""
    items = specials + families[0]
    return (items,) + _pack(items)


# ---------------------------------------------------------------- ecrecover
def test_ladder_exceptional_scalars(ctx, oracle, specials, exceptional):
    msgs, sigs = _pack(specials)
    ns = len(specials)
    assert ns == 24 * len(exceptional)
    want = np.array([_pub65(M.recover_expected(*it)) for it in specials])  # Python integers, every special
    # (1) among ordinary signatures: each special at lanes 0, 63, 64 and 255 of a 256-thread block in turn
    #     (the rare branch is wave-uniform: lanes 0 and 63 share a wave, 64 and 255 sit alone in theirs)
    lanes = (0, 63, 64, 255)
    nblk = ns
    bm, bs, _, _ = ctx.synth_sign(seed=606, n=256 * nblk, want_pub=False, want_addr=False)
    bm, bs = bm.copy(), bs.copy()
    where = np.zeros((nblk, 4), np.int64)
    for b in range(nblk):
        for k, lane in enumerate(lanes):
            i = (b + k * (ns // 4 + 1)) % ns
            where[b, k] = i
            bm[256 * b + lane], bs[256 * b + lane] = msgs[i], sigs[i]
    assert all((where == i).sum() == 4 and set(np.nonzero(where == i)[1]) == {0, 1, 2, 3} for i in range(ns))
    pub, addr, st = ctx.ecrecover_batch(bm, bs, want_pub=True, want_addr=True)
    _check_against_oracle(oracle, bm, bs, pub, addr, st)
    for b in range(nblk):
        for k, lane in enumerate(lanes):
            assert (pub[256 * b + lane] == want[where[b, k]]).all(), (b, lane)
    # (2) alone: a batch of one each (a lone lane in a lone wave)
    for i in range(ns):
        p1, a1, s1 = ctx.ecrecover_batch(msgs[i:i + 1], sigs[i:i + 1], want_pub=True, want_addr=True)
        assert s1[0] == ST_OK and (p1[0] == want[i]).all(), i
        assert bytes(a1[0]) == oracle.keccak256(bytes(want[i, 1:]))[12:], i
    # (3) together: every lane of the wave takes the exceptional branch
    pub, addr, st = ctx.ecrecover_batch(msgs, sigs, want_pub=True, want_addr=True)
    _check_against_oracle(oracle, msgs, sigs, pub, addr, st)
    assert (pub == want).all() and (addr == _addresses(oracle, want)).all()


def test_small_and_lattice_u2(ctx, oracle, families):
    items, n_small = families
    msgs, sigs = _pack(items)
    pub, addr, st = ctx.ecrecover_batch(msgs, sigs, want_pub=True, want_addr=True)
    _check_against_oracle(oracle, msgs, sigs, pub, addr, st)
    # Python integers on a seeded sample of both families
    rng = random.Random(64)
    sample = sorted(rng.sample(range(n_small), 40) + rng.sample(range(n_small, len(items)), 40))
    for i in sample:
        assert (pub[i] == _pub65(M.recover_expected(*items[i]))).all(), i


# ---------------------------------------------------------------- the other kernels that inline recover_core
@pytest.fixture(scope="module")
def plain_expected(oracle, crafted):
    """oracle_recover_plain (V = 27 + recid) for the crafted set: {homestead: (status, addr)}"""
    _, msgs, sigs = crafted
    L = oracle.lib()
    n = msgs.shape[0]
    rows = [(bytes(msgs[i]), bytes(sigs[i, :32]), bytes(sigs[i, 32:64]), bytes([27 + sigs[i, 64]])) for i in range(n)]
    out = {}
    for homestead in (0, 1):
        st = np.zeros(n, np.uint8)
        addr = np.zeros((n, 20), np.uint8)

        def one(i):
            buf = ctypes.create_string_buffer(20)
            m, r, s, v = rows[i]
            st[i] = L.oracle_recover_plain(buf, m, r, 32, s, 32, v, 1, homestead)
            if st[i] == 0:
                addr[i] = np.frombuffer(buf.raw, np.uint8)

        with ThreadPoolExecutor(8) as ex:  # the C call runs without the interpreter lock
            list(ex.map(one, range(n), chunksize=256))
        out[homestead] = (st, addr)
    return out


def test_crafted_through_sender_batch(ctx, crafted, plain_expected):
    _, msgs, sigs = crafted
    V = sigs[:, 64].astype(np.uint64) + 27
    VB = np.zeros(len(V), np.uint8)
    for homestead in (False, True):
        want_st, want_addr = plain_expected[int(homestead)]
        addr, st = ctx.sender_batch(msgs, sigs[:, :32], sigs[:, 32:64], V, VB, homestead)
        assert (st == want_st).all(), (homestead, np.nonzero(st != want_st)[0][:10])
        assert (addr[st == 0] == want_addr[st == 0]).all(), homestead
        high = np.array([int.from_bytes(bytes(s), "big") > M.HALF_N for s in sigs[:, 32:64]])
        assert (st[~high] == ST_OK).all()
        assert (st[high] == (ST_INVALID_SIG if homestead else ST_OK)).all() and high.any() and not high.all()


def test_crafted_through_precompile(ctx, crafted, plain_expected):
    _, msgs, sigs = crafted
    want_st, want_addr = plain_expected[0]
    assert (want_st == ST_OK).all()
    inputs = [bytes(msgs[i]) + bytes(31) + bytes([27 + sigs[i, 64]]) + bytes(sigs[i, :64]) for i in range(len(msgs))]
    out, ok = ctx.ecrecover_precompile_batch(inputs)
    assert ok.all(), np.nonzero(ok == 0)[0][:10]
    assert not out[:, :12].any() and (out[:, 12:] == want_addr).all()


def _crafted_tx(oracle, rng, nonce, u2, chain_id):
    """a transaction whose signature fields are (r, s) = (x_R, u2 x_R) with s <= n/2 (valid under every
    signer); chain_id None: unprotected (V = 27 + parity), else EIP-155.  The hash, hence u1, is what it is."""
    R = _random_point(rng, want_low_s_for=u2)
    r, s = R[0], u2 * R[0] % N
    data = bytes(rng.getrandbits(8) for _ in range(rng.randrange(0, 40)))
    fields = (oracle.rlp_uint(nonce) + oracle.rlp_uint(20 * 10 ** 9) + oracle.rlp_uint(21000 + len(data)) +
              oracle.rlp_string(bytes(range(1, 21))) + oracle.rlp_uint(10 ** 18 + nonce) + oracle.rlp_string(data))
    v = (R[1] & 1) + (27 if chain_id is None else 35 + 2 * chain_id)
    return oracle.rlp_list(fields + oracle.rlp_uint(v) + oracle.rlp_uint(r) + oracle.rlp_uint(s))


def test_crafted_through_notary_and_tx_sender(ctx, oracle, exceptional):
    rng = random.Random(0x7a)
    small = [u for u, _, _ in M.small_family(40)]
    scalars = exceptional + rng.sample(small, 64)
    chain_id = 1
    txs = []
    for i, u2 in enumerate(scalars):
        txs.append(_crafted_tx(oracle, rng, 2 * i, u2, chain_id))
        txs.append(_crafted_tx(oracle, rng, 2 * i + 1, u2, None))
    body = oracle.blob_serialize(txs)
    max_txs = 256
    assert len(txs) <= max_txs
    for signer in (0, 1, 2):  # EIP155Signer(1), HomesteadSigner, FrontierSigner
        want = [oracle.tx_sender(t, chain_id, signer) for t in txs]
        if signer == 0:
            assert all(s == ST_OK for s, _ in want)
        assert all(s == ST_OK for s, _ in want[1::2])  # the unprotected ones: valid under every signer
        _, ntx, bitmap, senders, status = ctx.notary_validate_shards([body], chain_id, signer, max_txs)
        addr, st = ctx.tx_sender_batch(txs, chain_id, signer)
        assert ntx[0] == len(txs)
        for t, (s, a) in enumerate(want):
            assert status[0, t] == s and st[t] == s, (signer, t, status[0, t], st[t], s)
            assert ((bitmap[0, t // 8] >> (t % 8)) & 1) == (s == ST_OK)
            if s == ST_OK:
                assert bytes(senders[0, t]) == a and bytes(addr[t]) == a, (signer, t)


# ---------------------------------------------------------------- every reachable entry of the comb table
def _window_r(w):
    """(t, R_w): the smallest t >= 1 for which r = t 2^(-COMB_BITS w) mod n is a curve x, and that point (y even)"""
    inv = pow(pow(2, M.COMB_BITS * w, N), -1, N)
    for t in range(1, 64):
        R = M.lift_x(t * inv % N, 0)
        if R is not None:
            return t, R
    raise AssertionError("no x-coordinate among the first multiples")


@pytest.mark.parametrize("w", range(M.COMB_WINDOWS))
def test_comb_table_every_entry(ctx, oracle, w):
    """Item d has msg = n - d t and r = t 2^(-COMB_BITS w): u1 = -msg / r = d 2^(COMB_BITS w) exactly, so the
    comb reads entry (w, d) and otherwise only the d = 0 entries, which it skips.  One launch covers every
    d of the window.  In the top window d stops at (n - 1) >> (COMB_BITS w): a larger d would make u1 >= n,
    so the entries above it are reachable by no input (u1 is reduced mod n before the comb) and are not
    tested here."""
    bits = M.COMB_BITS
    t, R = _window_r(w)
    count = min(1 << bits, ((N - 1) >> (bits * w)) + 1)
    assert count == (1 << bits) or w == M.COMB_WINDOWS - 1
    n_lo = N & (2 ** 64 - 1)
    assert n_lo > (t << bits)  # msg = n - d t stays inside the low 64 bits
    u2 = random.Random(1000 + w).randrange(1, N)
    d = np.arange(count, dtype=np.uint64)
    msgs = np.empty((count, 32), np.uint8)
    msgs[:, :24] = np.frombuffer(_be32(N)[:24], np.uint8)
    msgs[:, 24:] = (np.uint64(n_lo) - d * np.uint64(t)).astype(">u8").view(np.uint8).reshape(count, 8)
    sig = _be32(R[0]) + _be32(u2 * R[0] % N) + bytes([R[1] & 1])
    sigs = np.broadcast_to(np.frombuffer(sig, np.uint8), (count, 65)).copy()
    for dd in (0, 1, count - 1):  # the vectorised messages against Python integers
        assert bytes(msgs[dd]) == _be32(N - dd * t)
        assert M.comb_digits((-(N - dd * t) * pow(R[0], -1, N)) % N) == [dd if k == w else 0 for k in range(M.COMB_WINDOWS)]
    pub, _, st = ctx.ecrecover_batch(msgs, sigs, want_pub=True, want_addr=False)
    assert (st == ST_OK).all(), np.nonzero(st != ST_OK)[0][:10]
    assert (pub[:, 0] == 4).all()
    base = M.ec_mul(1 << (bits * w), M.G)
    rc = oracle.secp_chain_check(pub[:, 1:], _be32(base[0]) + _be32(base[1]), threads=16)
    assert rc != oracle.CHAIN_DEGENERATE  # no Q[d-1] shares its x with the base
    assert rc == oracle.CHAIN_OK, "entry (%d, %d): Q[d] != Q[d-1] + 2^(%d) G" % (w, rc, bits * w)
    # the chain's anchor by Python integers, and sampled links (the second and the last among them) by the oracle
    assert (pub[0] == _pub65(M.ec_mul(u2, R))).all()
    rng = random.Random(2000 + w)
    pick = np.array(sorted({1, count - 1} | {rng.randrange(2, count - 1) for _ in range(8)}))
    opub, ost = oracle.ecrecover_batch(msgs[pick], sigs[pick])
    assert (ost == ST_OK).all() and (pub[pick] == opub).all()
