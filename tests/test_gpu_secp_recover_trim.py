"""GPU parity of the recovery's prologue, the starts of its two sums and its exceptional-case filter
(secp256k1_glv.cuh, secp256k1_comb.cuh: digits read from the scalar's bits, the affine + affine first
adds, the comb's adds without a test, the one-limb filter, the split's short products), on crafted signatures (r = x_R,
s = u2 r, msg = -u1 r: tests/secp_glv_model.py craft) through the four kernels that inline recover_core,
at batch sizes 1, 63, 64, 65 and 257 (a lone lane, a ragged wave, a full one, a second wave, a second
block), bit-exact against the oracle, the doubling case also against Python integers.

The crafted scalars:
  * u1 with its low 20 bits zero (the comb's identity start reaches the peeled window-1 add), its low 40
    bits zero (window 1 is skipped too) and u1 = 0 (the identity goes into the tail), beside random u1;
  * u2 whose halves carry every 4-bit pattern in their lowest digit and in their highest full digit
    (slot GLV_DIGITS - 2; the top digit above it has one bit), as far as the model finds
    them among 10^5 candidates: all 16 low patterns of both halves, all 16 high patterns of the first
    half, 0..11 of the second (its magnitude stays below 1.5 2^128);
  * the top digits: both halves stay below 2^129 for every scalar (|k1| <= (|a1| + |a2|) / 2 + |a2|,
    |k2| <= (|b1| + |b2|) / 2 + |b1| after glv_make_odd), so the top digits are (1, 1) always: the model
    finds no (1, 3), (3, 1) or (3, 3) among the candidates (asserted), and the items with the largest
    first and second halves it found stand in for them;
  * u2 = -26 lambda, the ladder's one doubling: alone (batch of one), in a wave of ordinary items, and
    in a wave where every lane doubles.  It must still reach the out-of-line doubling through the filter.
The notary kernel hashes its transactions itself, so u1 is what the hash makes it there; u2 is crafted."""
import ctypes
import random

import numpy as np
import pytest

import secp_glv_model as M
from test_gpu_secp256k1_scalars import (ST_OK, U2_DOUBLING, _addresses, _check_against_oracle, _crafted_tx, _pack,
                                        _pub65, _random_point)

pytestmark = pytest.mark.gpu
N, LAM = M.N, M.LAMBDA
SIZES = (1, 63, 64, 65, 257)
TOP = M.GLV_DIGITS - 1
SLOT_MASK = (1 << M.GLV_W) - 1


def _halves(u2):
    k1, k2, _ = M.make_odd(*M.split_lambda(u2))
    return M.magnitude(k1)[1], M.magnitude(k2)[1]


@pytest.fixture(scope="module")
def crafted_u2():
    """one u2 per (half, digit position, pattern) the model finds among 10^5 candidates (half of them
    uniform, half a + b lambda with |a|, |b| in [2^126, 2^128): the large halves), then the candidates
    with the largest halves"""
    rng = random.Random(0x7e57)
    cands = [rng.randrange(1, N) for _ in range(50000)]
    for _ in range(50000):
        a = rng.randrange(1 << 126, 1 << 128) * rng.choice((1, -1))
        b = rng.randrange(1 << 126, 1 << 128) * rng.choice((1, -1))
        cands.append((a + b * LAM) % N)
    found, tops, largest = {}, set(), [(0, 0), (0, 0)]
    for u in cands:
        mags = _halves(u)
        tops.add(tuple(2 * (m >> (M.GLV_W * TOP + 1)) + 1 for m in mags))
        for h, m in enumerate(mags):
            K = m >> 1
            found.setdefault((h, 0, K & SLOT_MASK), u)
            found.setdefault((h, TOP - 1, (K >> (M.GLV_W * (TOP - 1))) & SLOT_MASK), u)
            largest[h] = max(largest[h], (m, u))
    assert tops == {(1, 1)}  # no half reaches 2^129: the top digit is 1 for both, always
    for h in (0, 1):
        assert {p for (hh, i, p) in found if hh == h and i == 0} == set(range(16))
    assert {p for (hh, i, p) in found if hh == 0 and i == TOP - 1} == set(range(16))
    assert {p for (hh, i, p) in found if hh == 1 and i == TOP - 1} == set(range(12))
    assert largest[0][0] >> 128 and largest[1][0] >> 128
    return [found[k] for k in sorted(found)] + [largest[0][1], largest[1][1]]


@pytest.fixture(scope="module")
def items(crafted_u2):
    """every crafted u2 with each kind of u1, the doubling first: [(R, u1, u2)]"""
    rng = random.Random(0x17e5)
    pool = [_random_point(rng) for _ in range(8)]
    u1s = lambda: (rng.randrange(1, N), (rng.randrange(1, N >> 20) << 20) % N, (rng.randrange(1, N >> 40) << 40) % N, 0)
    out = [(pool[0], rng.randrange(1, N), U2_DOUBLING)]
    for i, u2 in enumerate(crafted_u2):
        out += [(pool[(i + j) % 8], u1, u2) for j, u1 in enumerate(u1s())]
    assert all(M.comb_digits(it[1])[0] == 0 for it in out[2::4])
    assert all(M.comb_digits(it[1])[:2] == [0, 0] for it in out[3::4]) and all(it[1] == 0 for it in out[4::4])
    return out


def _batches(items):
    """for every size: the doubling at lane 0, then a rotating slice of the others (every item is in some batch)"""
    rest, off, out = items[1:], 0, []
    assert sum(n - 1 for n in SIZES) >= len(rest)
    for n in SIZES:
        out.append([items[0]] + [rest[(off + k) % len(rest)] for k in range(n - 1)])
        off += n - 1
    return out


@pytest.fixture(scope="module")
def batches(items):
    return [(b,) + _pack(b) for b in _batches(items)]


def test_ecrecover_at_every_batch_size(ctx, oracle, batches):
    for b, msgs, sigs in batches:
        pub, addr, st = ctx.ecrecover_batch(msgs, sigs, want_pub=True, want_addr=True)
        _check_against_oracle(oracle, msgs, sigs, pub, addr, st)
        assert (pub[0] == _pub65(M.recover_expected(*b[0]))).all(), len(b)  # the doubling, by Python integers
        for i in range(1, len(b), 37):
            assert (pub[i] == _pub65(M.recover_expected(*b[i]))).all(), (len(b), i)


def test_doubling_in_every_lane_of_a_wave(ctx, oracle):
    rng = random.Random(0xdb1)
    b = [(_random_point(rng), rng.randrange(0, N) if k % 3 else 0, U2_DOUBLING) for k in range(64)]
    msgs, sigs = _pack(b)
    pub, addr, st = ctx.ecrecover_batch(msgs, sigs, want_pub=True, want_addr=True)
    _check_against_oracle(oracle, msgs, sigs, pub, addr, st)
    want = np.array([_pub65(M.recover_expected(*it)) for it in b])
    assert (pub == want).all() and (addr == _addresses(oracle, want)).all()


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


def test_sender_and_precompile_at_every_batch_size(ctx, oracle, batches):
    for b, msgs, sigs in batches:
        n = len(b)
        want_st, want_addr = _plain(oracle, msgs, sigs, 0)
        assert (want_st == ST_OK).all()
        V = sigs[:, 64].astype(np.uint64) + 27
        addr, st = ctx.sender_batch(msgs, sigs[:, :32], sigs[:, 32:64], V, np.zeros(n, np.uint8), False)
        assert (st == want_st).all() and (addr == want_addr).all(), n
        hst, haddr = _plain(oracle, msgs, sigs, 1)
        addr, st = ctx.sender_batch(msgs, sigs[:, :32], sigs[:, 32:64], V, np.zeros(n, np.uint8), True)
        assert (st == hst).all() and (addr[st == 0] == haddr[st == 0]).all(), n
        inputs = [bytes(msgs[i]) + bytes(31) + bytes([27 + sigs[i, 64]]) + bytes(sigs[i, :64]) for i in range(n)]
        out, ok = ctx.ecrecover_precompile_batch(inputs)
        assert ok.all() and not out[:, :12].any() and (out[:, 12:] == want_addr).all(), n


def test_notary_at_every_batch_size(ctx, oracle, items):
    rng = random.Random(0x7a2)
    chain_id = 1
    for b in _batches(items):
        n = len(b)
        txs = [_crafted_tx(oracle, rng, i, it[2], chain_id if i % 2 else None) for i, it in enumerate(b)]
        want = [oracle.tx_sender(t, chain_id, 0) for t in txs]
        assert all(s == ST_OK for s, _ in want)
        max_txs = (n + 7) // 8 * 8
        _, ntx, bitmap, senders, status = ctx.notary_validate_shards([oracle.blob_serialize(txs)], chain_id, 0, max_txs)
        addr, st = ctx.tx_sender_batch(txs, chain_id, 0)
        assert ntx[0] == n
        for t, (s, a) in enumerate(want):
            assert status[0, t] == s and st[t] == s, (n, t)
            assert (bitmap[0, t // 8] >> (t % 8)) & 1
            assert bytes(senders[0, t]) == a and bytes(addr[t]) == a, (n, t)
