"""GPU parity of batched types.SignTx (k_tx_sighash, k_ecsign, k_tx_seal behind gsv_tx_sign_batch and
gsv_tx_sign_batch_dev) with the model tests/tx_sign_model.py run with the reference's own signer
(oracle.ref().gsvref_sign) and oracle.keccak256.  Every comparison is byte for byte on out[slot : slot + len],
out_len, the hash and the status, through the host form and the device-resident form; every device run
checks the guard bytes before the first slot, behind the last, in every slot's unused tail and behind
out_len, hash and status."""
import ctypes

import numpy as np
import pytest

import tx_rules_corpus as RC
import tx_rules_model as M
import tx_sign_corpus as C
import tx_sign_model as S
from conftest import golden

pytestmark = pytest.mark.gpu
GUARD = 0xEE
PAD = 61  # guard bytes before the first slot and before the first transaction: odd, so nothing is aligned


def keyrows(keys):
    return np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 32).copy()


def growth(cid):
    return S.growth(len(C.be(cid)))


class DevRun:
    """the device form on one explicit stream over guarded buffers"""

    def __init__(self, ctx, blobs, keys, signer, cid, want_hash=True):
        import torch
        import gsv
        self.ctx, self.signer, self.cid, self.n = ctx, signer, cid, len(blobs)
        dev = torch.device("cuda", ctx.device)
        n, G = self.n, growth(cid)
        self.off = np.zeros(n + 1, np.int64)
        np.cumsum([len(b) for b in blobs], out=self.off[1:])
        total = int(self.off[n])
        flat = np.full(PAD + total + 8, GUARD, np.uint8)
        flat[PAD:PAD + total] = np.frombuffer(b"".join(blobs), np.uint8)
        self.d_rlp = torch.from_numpy(flat).to(dev)
        self.d_off = torch.from_numpy(self.off).to(dev)
        self.d_key = torch.from_numpy(keyrows(keys) if n else np.zeros((0, 32), np.uint8)).to(dev)
        self.out_bytes = total + n * G
        self.d_out = torch.full((PAD + self.out_bytes + 64,), GUARD, dtype=torch.uint8, device=dev)
        self.d_olen = torch.full((n + 1,), 0x6E6E6E6E, dtype=torch.int32, device=dev)
        self.d_hash = torch.full((n + 1, 32), GUARD, dtype=torch.uint8, device=dev) if want_hash else None
        self.d_st = torch.full((n + 1,), GUARD, dtype=torch.uint8, device=dev)
        self.d_work = torch.zeros((gsv.tx_sign_work_bytes(n) + 16,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

    def enqueue(self, stream):
        self.ctx.tx_sign_batch_dev(self.d_rlp[PAD:], self.d_off, self.d_key, self.cid, self.signer, self.d_out[PAD:],
                                   self.d_olen[:self.n], self.d_hash[:self.n] if self.d_hash is not None else None,
                                   self.d_st[:self.n], self.d_work, stream=stream)

    def run(self):
        import torch
        cs = torch.cuda.Stream()
        self.enqueue(cs)
        cs.synchronize()
        return self

    def check(self, exp, blobs):
        """exp: [(status, signed, hash)] of the model"""
        n, G = self.n, growth(self.cid)
        out = self.d_out.cpu().numpy()
        olen = self.d_olen.cpu().numpy()
        st = self.d_st.cpu().numpy()
        assert (out[:PAD] == GUARD).all() and (out[PAD + self.out_bytes:] == GUARD).all(), "bytes outside the slots"
        assert olen[n] == 0x6E6E6E6E and st[n] == GUARD
        assert [int(x) for x in st[:n]] == [e[0] for e in exp], np.nonzero(st[:n] != np.array([e[0] for e in exp]))[0][:10]
        assert [int(x) for x in olen[:n]] == [len(e[1]) for e in exp]
        for i, e in enumerate(exp):
            lo = PAD + int(self.off[i]) + i * G
            hi = PAD + int(self.off[i + 1]) + (i + 1) * G
            assert out[lo:lo + len(e[1])].tobytes() == e[1], (i, blobs[i].hex())
            assert (out[lo + len(e[1]):hi] == GUARD).all(), ("slot tail", i)
        if self.d_hash is not None:
            h = self.d_hash.cpu().numpy()
            assert (h[n] == GUARD).all()
            assert h[:n].tobytes() == b"".join(e[2] for e in exp)
        return self


def host_check(ctx, blobs, keys, signer, cid, exp):
    signed, hashes, st = ctx.tx_sign_batch(blobs, keyrows(keys), cid, signer)
    assert [int(x) for x in st] == [e[0] for e in exp]
    assert signed == [e[1] for e in exp]
    assert hashes.tobytes() == b"".join(e[2] for e in exp)


def by_group(items):
    """{(signer, chain id): [index]} in first-seen order"""
    g = {}
    for i, (_, _, s, c) in enumerate(items):
        g.setdefault((s, c), []).append(i)
    return g


@pytest.fixture(scope="module")
def bulk(oracle):
    """the 4,096 seeded transactions and the model's results with the reference's signer, computed once"""
    items = C.differential()
    return items, C.expected(oracle, items)


# ---------------------------------------------------------------- 1. recorded rows
def test_fixture_rows_host_and_dev(ctx, oracle):
    rows = golden("tx_sign.json")["rows"]
    items = [(bytes.fromhex(r["rlp"]), bytes.fromhex(r["key"]), r["signer"], int(r["chain_id"], 16)) for r in rows]
    exp = [(r["status"], bytes.fromhex(r["signed"]), bytes.fromhex(r["hash"])) for r in rows]
    assert exp == C.expected(oracle, items)  # the file against the reference's signer, here and now
    for (signer, cid), idx in by_group(items).items():
        blobs, keys, e = [items[i][0] for i in idx], [items[i][1] for i in idx], [exp[i] for i in idx]
        host_check(ctx, blobs, keys, signer, cid, e)
        DevRun(ctx, blobs, keys, signer, cid).run().check(e, blobs)
    # the types mirror, one item at a time
    from gsv import types
    r = rows[0]
    assert types.SignTx(bytes.fromhex(r["rlp"]), types.EIP155Signer(1), int(r["key"], 16), ctx).hex() == r["signed"]
    r = next(r for r in rows if r["signer"] == M.SIGNER_FRONTIER)
    assert types.SignTx(bytes.fromhex(r["rlp"]), types.FrontierSigner(), bytes.fromhex(r["key"]), ctx).hex() == r["signed"]
    with pytest.raises(types.ErrInvalidKey, match="invalid private key"):
        types.SignTx(bytes.fromhex(r["rlp"]), types.HomesteadSigner(), 0, ctx)
    with pytest.raises(types.ErrBadRLP):
        types.SignTx(bytes.fromhex(r["rlp"]) + b"\0", types.HomesteadSigner(), 1, ctx)


# ---------------------------------------------------------------- 2. differential
def test_differential_4096(ctx, oracle, bulk):
    items, exp = bulk
    assert len(items) == 4096 and all(e[0] == S.ST_OK for e in exp)
    groups = by_group(items)
    assert list(groups) == list(C.GROUPS)
    for (signer, cid), idx in groups.items():
        blobs, keys, e = [items[i][0] for i in idx], [items[i][1] for i in idx], [exp[i] for i in idx]
        host_check(ctx, blobs, keys, signer, cid, e)
        DevRun(ctx, blobs, keys, signer, cid).run().check(e, blobs)


def test_signed_input_signs_to_the_same_output(ctx, bulk):
    """the model's outputs of one group, fed back with the same keys: SignTx ignores the signature it finds"""
    items, exp = bulk
    for signer, cid in ((M.SIGNER_EIP155, C.C64T), (M.SIGNER_EIP155, 46), (M.SIGNER_FRONTIER, 1)):
        idx = by_group(items)[(signer, cid)][:130]
        signed_in, keys, e = [exp[i][1] for i in idx], [items[i][1] for i in idx], [exp[i] for i in idx]
        assert all(a != items[i][0] for a, i in zip(signed_in, idx))
        host_check(ctx, signed_in, keys, signer, cid, e)
        DevRun(ctx, signed_in, keys, signer, cid).run().check(e, signed_in)


# ---------------------------------------------------------------- 3. launch shapes
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_launch_shapes(ctx, bulk, n):
    items, exp = bulk
    signer, cid = C.GROUPS[1]
    idx = by_group(items)[(signer, cid)][:n]
    assert len(idx) == n
    blobs, keys, e = [items[i][0] for i in idx], [items[i][1] for i in idx], [exp[i] for i in idx]
    DevRun(ctx, blobs, keys, signer, cid).run().check(e, blobs)
    DevRun(ctx, blobs, keys, signer, cid, want_hash=False).run().check(e, blobs)
    host_check(ctx, blobs, keys, signer, cid, e)
    if n == 0:
        from gsv import _lib
        L = _lib.load()
        assert L.gsv_tx_sign_batch(ctx.handle, None, None, 0, None, None, 0, 0, None, None, None, None) == 0
        assert L.gsv_tx_sign_batch_dev(ctx.handle, None, None, 0, None, None, 0, 0, None, None, None, None, None, None) == 0


# ---------------------------------------------------------------- 4. statuses
@pytest.mark.parametrize("chain_id", RC.CHAIN_IDS)
def test_rules_corpus_statuses(ctx, oracle, chain_id):
    """every case of tests/tx_rules_corpus.py: BAD_RLP exactly where the model's decode fails, OK and the
    model's bytes elsewhere, the corpus's invalid signatures and wrong chain ids included"""
    cases = RC.build(oracle, chain_id)
    blobs = [c.blob for c in cases]
    keys = [RC.KEY] * len(blobs)
    sign = C.ref_signer(oracle)
    want_bad = [_decodes(b) is False for b in blobs]
    assert 200 < sum(want_bad) < len(blobs) - 200
    cache = {}
    for signer in RC.SIGNERS:
        hk = signer == M.SIGNER_EIP155  # Homestead and Frontier hash alike
        if hk not in cache:
            cache[hk] = [S.sign_tx(b, RC.KEY, signer, chain_id, sign, oracle.keccak256) for b in blobs]
        exp = cache[hk]
        assert [e[0] == S.ST_BAD_RLP for e in exp] == want_bad and {e[0] for e in exp} == {S.ST_OK, S.ST_BAD_RLP}
        DevRun(ctx, blobs, keys, signer, chain_id).run().check(exp, blobs)
        if signer == M.SIGNER_EIP155:
            host_check(ctx, blobs, keys, signer, chain_id, exp)
    # the corpus's invalid-signature and wrong-chain-id cases sign normally
    addr, sst = ctx.tx_sender_batch(blobs, chain_id, M.SIGNER_EIP155)
    resigned = [e[0] for e, s in zip(cache[True], sst) if s in (M.ST_INVALID_SIG, M.ST_INVALID_CHAIN_ID, M.ST_RECOVER_FAILED)]
    assert len(resigned) > 50 and set(resigned) == {S.ST_OK}


def _decodes(blob):
    try:
        M.decode_txdata(blob)
        return True
    except M.RLPError:
        return False


def test_key_rule_precedence_and_size_limit(ctx, oracle, bulk):
    from gsv import _lib
    items, exp = bulk
    signer, cid = C.GROUPS[1]
    idx = (by_group(items)[(signer, cid)] * 2)[:64 * 7]  # seven waves
    assert len(idx) == 64 * 7
    blobs, keys, e = [items[i][0] for i in idx], [items[i][1] for i in idx], [exp[i] for i in idx]
    sign = C.ref_signer(oracle)
    big = S.unsigned_tx(1, 1, 21000, C.TO, 1, bytes(range(1, 256)) * 4113)
    assert len(big) > (1 << 20) and _decodes(big)
    most = S.unsigned_tx(1, 1, 21000, C.TO, 1, bytes((1 << 20) - 38))
    assert len(most) == 1 << 20
    bad = {64 * 0 + 3: (blobs[3], bytes(32)),                                  # key 0
           64 * 1 + 17: (blobs[81], M.SECP_N.to_bytes(32, "big")),              # key n
           64 * 2 + 63: (blobs[191], b"\xff" * 32),                             # key 2^256 - 1
           64 * 3 + 0: (blobs[192] + b"\x00", bytes(32)),                       # both faults: BAD_RLP
           64 * 4 + 31: (big, keys[287]),                                       # past 2^20 bytes
           64 * 5 + 32: (big[:-1] + b"\x00\x00", bytes(32)),                    # ... whatever it holds
           64 * 6 + 1: (most, keys[385])}                                       # exactly 2^20 bytes: signed
    for k, (b, key) in bad.items():
        blobs[k], keys[k] = b, key
        e[k] = S.sign_tx(b, key, signer, cid, sign, oracle.keccak256)
    assert [e[k][0] for k in bad] == [_lib.ST_INVALID_KEY] * 3 + [_lib.ST_BAD_RLP] + [_lib.ST_BODY_TOO_LARGE] * 2 + [0]
    assert [e[k][0] for k in bad] == [11, 11, 11, 8, 13, 13, 0]
    # check(): failing items have out_len 0, a zero hash and an untouched slot; their neighbours are correct
    DevRun(ctx, blobs, keys, signer, cid).run().check(e, blobs)
    host_check(ctx, blobs, keys, signer, cid, e)
    # whole waves of failing items
    z = [blobs[0]] * 65
    DevRun(ctx, z, [bytes(32)] * 65, signer, cid).run().check([(11, b"", bytes(32))] * 65, z)
    z = [b"\xc0"] * 65
    DevRun(ctx, z, keys[:65], signer, cid).run().check([(8, b"", bytes(32))] * 65, z)


# ---------------------------------------------------------------- 5. guard bytes of the host form
def test_host_form_writes_only_its_items(ctx, bulk):
    from gsv import _lib
    items, exp = bulk
    signer, cid = C.GROUPS[7]
    idx = by_group(items)[(signer, cid)][:100]
    blobs, e = [items[i][0] for i in idx], [exp[i] for i in idx]
    keys = keyrows([items[i][1] for i in idx])
    keys[40] = 0  # a failing item: its slot stays as it was
    e[40] = (11, b"", bytes(32))
    n, G, base = len(blobs), growth(cid), 24  # the caller's table need not start at 0
    off = np.zeros(n + 1, np.uint64)
    off[0] = base
    off[1:] = base + np.cumsum([len(b) for b in blobs])
    flat = np.frombuffer(bytes(base) + b"".join(blobs) + bytes(8), np.uint8)
    out = np.full(int(off[n]) + n * G + 32, GUARD, np.uint8)
    olen = np.full(n + 1, 0x6E6E6E6E, np.uint32)
    h = np.full((n + 1, 32), GUARD, np.uint8)
    st = np.full(n + 1, GUARD, np.uint8)
    cidb = np.frombuffer(C.be(cid), np.uint8)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    rc = _lib.load().gsv_tx_sign_batch(ctx.handle, p(flat), p(off), n, p(keys), p(cidb), cidb.size, signer, p(out),
                                       p(olen), p(h), p(st))
    assert rc == 0
    assert olen[n] == 0x6E6E6E6E and (h[n] == GUARD).all() and st[n] == GUARD
    assert (out[:base] == GUARD).all() and (out[int(off[n]) + n * G:] == GUARD).all()
    for i in range(n):
        lo, hi = int(off[i]) + i * G, int(off[i + 1]) + (i + 1) * G
        assert out[lo:lo + olen[i]].tobytes() == e[i][1] and (out[lo + olen[i]:hi] == GUARD).all(), i
        assert st[i] == e[i][0] and h[i].tobytes() == e[i][2]


# ---------------------------------------------------------------- 6. round trips
def test_sender_recovers_the_signing_key(ctx, oracle, bulk):
    items, exp = bulk
    for (signer, cid), idx in by_group(items).items():
        idx = idx[:96]
        _, addr, st = ctx.pubkey_create_batch(keyrows([items[i][1] for i in idx]), want_addr=True)
        assert (st == 0).all()
        signed, _, sst = ctx.tx_sign_batch([items[i][0] for i in idx], keyrows([items[i][1] for i in idx]), cid, signer)
        assert (sst == 0).all()
        got, rst = ctx.tx_sender_batch(signed, cid, signer)
        if C.sender_is_inverse(signer, cid):
            assert (rst == 0).all() and (got == addr).all(), (signer, cid)
            for k in (0, 50, 95):  # and the oracle's types.Sender
                assert oracle.tx_sender(signed[k], cid, signer) == (0, bytes(addr[k]))
        else:  # tests/tx_sign_corpus.py sender_is_inverse: the signature is pinned over the hash that was signed
            assert not ((rst == 0) & (got == addr).all(axis=1)).any()
            for k in range(0, 96, 5):
                assert C.signer_address(oracle, signed[k], signer, cid) == bytes(addr[k])


def test_sign_collate_validate(ctx, oracle):
    """2 x 64 unsigned transactions: SignTx, CreateCollations, the notary call"""
    import random
    from gsv import sharding, types
    rng = random.Random(0xc011)
    keys = [rng.randrange(1, M.SECP_N) for _ in range(128)]
    unsigned = [S.unsigned_tx(j % 64, 20 * 10 ** 9, 21000, C.TO if j % 5 else None, 10 ** 15 + j,
                              bytes(rng.getrandbits(8) for _ in range(j % 70)), to_as_list=j % 10 == 0) for j in range(128)]
    signed, hashes, st = types.SignTxBatch(unsigned, types.EIP155Signer(1), keys, ctx=ctx)
    assert (st == 0).all()
    assert all(bytes(h) == oracle.keccak256(t) for h, t in zip(hashes, signed))
    _, addr, _ = ctx.pubkey_create_batch(keyrows([k.to_bytes(32, "big") for k in keys]), want_addr=True)
    pkeys = [rng.randrange(1, M.SECP_N) for _ in range(2)]
    _, paddr, _ = ctx.pubkey_create_batch(keyrows([k.to_bytes(32, "big") for k in pkeys]), want_addr=True)
    cols = sharding.CreateCollations([signed[:64], signed[64:]], [3, 4], [10, 11], [bytes(a) for a in paddr], pkeys, ctx)
    roots, ntx, bitmap, senders, status = ctx.notary_validate_shards([c.Body() for c in cols], 1, M.SIGNER_EIP155, 64)
    for i, col in enumerate(cols):
        assert bytes(roots[i]) == col.Header().ChunkRoot() and ntx[i] == 64
        assert (status[i] == 0).all() and (bitmap[i] == 0xFF).all()
        assert (senders[i] == addr[64 * i:64 * i + 64]).all()
    signer, vst = sharding.VerifyProposerSignatures([c.Header() for c in cols], ctx)
    assert (vst == 0).all() and (signer == paddr).all()


# ---------------------------------------------------------------- 7. capture
def test_dev_form_is_capturable(ctx, oracle, bulk):
    import torch
    from gsv import _lib
    items, exp = bulk
    signer, cid = C.GROUPS[6]  # a 32-byte chain id: it travels in the kernels' arguments
    idx = by_group(items)[(signer, cid)][:257]
    blobs, keys, e = [items[i][0] for i in idx], [items[i][1] for i in idx], [exp[i] for i in idx]
    run = DevRun(ctx, blobs, keys, signer, cid)
    cs = torch.cuda.Stream()
    # three launches per call, timed under their ids
    ctx.set_timing(True)
    try:
        ctx.reset_timing()
        run.enqueue(cs)
        cs.synchronize()
        for kid in (_lib.K_TX_SIGHASH, _lib.K_ECRECOVER, _lib.K_TX_SEAL):
            ms, launches = ctx.kernel_time(kid)
            assert launches == 1 and ms > 0, kid
    finally:
        ctx.set_timing(False)
        ctx.reset_timing()
    run.check(e, blobs)
    # captured on an explicit stream (nothing allocated, nothing synchronised inside), replayed twice with
    # changed inputs: the keys of the first replay, then each key moved one item on
    g = torch.cuda.CUDAGraph()
    shapes_before = ctx.prepared_shapes()
    with torch.cuda.graph(g, stream=cs):
        run.enqueue(cs)
    assert ctx.prepared_shapes() == shapes_before
    sign_keys = [keys, keys[1:] + keys[:1]]
    sign = C.ref_signer(oracle)
    for ks in sign_keys:
        want = e if ks is keys else [S.sign_tx(b, k, signer, cid, sign, oracle.keccak256) for b, k in zip(blobs, ks)]
        run.d_key.copy_(torch.from_numpy(keyrows(ks)))
        run.d_out.fill_(GUARD)
        run.d_hash.fill_(GUARD)
        run.d_st.fill_(GUARD)
        run.d_olen.fill_(0x6E6E6E6E)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        run.check(want, blobs)


# ---------------------------------------------------------------- 8. secret hygiene
def test_staged_keys_are_wiped(ctx):
    """after the host form returns, the arena's key region (the first region: offset 0, 32 n bytes) holds none
    of the key bytes; the work area behind it still holds this call's records, so the read looks at the arena
    this call staged in"""
    n = 300
    keys = np.full((n, 32), 0xA5, np.uint8)
    blob = S.unsigned_tx(5, 20 * 10 ** 9, 21000, C.TO, 10 ** 18, b"\x01\x02")
    signed, _, st = ctx.tx_sign_batch([blob] * n, keys, 1, M.SIGNER_EIP155)
    assert (st == 0).all() and len(set(signed)) == 1 and len(signed[0]) > len(blob)
    assert not ctx._arena_read(0, n * 32).any(), "staged secret keys left in the arena"
    behind = (n * 32 + 255) // 256 * 256
    rec = ctx._arena_read(behind, n * 16).view(np.uint32).reshape(n, 4)
    # {segment offset, segment length, no recipient patch, status OK} of every item
    assert (rec == np.array([1, len(blob) - 4, 0xFFFFFFFF, 0], np.uint32)).all()
