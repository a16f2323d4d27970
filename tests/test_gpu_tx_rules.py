"""GPU parity with the reference's transaction decode and signer rules: the structured corpus of
tests/tx_rules_corpus.py through gsv_notary_validate_shards (k_blob_index + k_notary_tx, every header
byte read through the chunk map) and gsv_tx_sender_batch (host decode + k_sender), against the
independent model tests/tx_rules_model.py finished by oracle.ecrecover, and the blob index against the
model's Deserialize (sharding/utils/marshal.go:144-198) on bodies of more than 1,024 chunks.  Chunk
roots stay compared with oracle.derive_sha_bytes.  tests/test_tx_rules.py pins the model and runs the
same corpus through the CPU oracle and the host decoder."""
import numpy as np
import pytest

import tx_rules_corpus as C
import tx_rules_model as M

pytestmark = pytest.mark.gpu

PER_SHARD = 512  # transactions per shard body: the corpus is five bodies of at most 230 KB


@pytest.fixture(scope="module")
def corpora(oracle):
    out = {}
    for cid in C.CHAIN_IDS:
        cases = C.build(oracle, cid)
        shards = [cases[i:i + PER_SHARD] for i in range(0, len(cases), PER_SHARD)]
        bodies = [M.serialize([c.blob for c in s]) for s in shards]
        assert all(len(b) <= 1 << 20 for b in bodies)
        out[cid] = (cases, bodies, [oracle.derive_sha_bytes(b) for b in bodies])
    return out


def _validate_dev(ctx, body, max_txs):
    """gsv_notary_validate_shards_dev on one body (chain id 1, EIP-155 signer), results as numpy arrays"""
    import torch
    b_t = torch.zeros(len(body) + 64, dtype=torch.uint8, device="cuda")  # zero bytes after the body
    b_t[:len(body)] = torch.frombuffer(bytearray(body), dtype=torch.uint8).cuda()
    r_t = torch.zeros((1, 32), dtype=torch.uint8, device="cuda")
    n_t = torch.zeros((1,), dtype=torch.int32, device="cuda")
    m_t = torch.zeros((1, (max_txs + 7) // 8), dtype=torch.uint8, device="cuda")
    a_t = torch.zeros((1, max_txs, 20), dtype=torch.uint8, device="cuda")
    s_t = torch.zeros((1, max_txs), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # the library enqueues on its own stream
    ctx.notary_validate_shards_dev(b_t, np.array([0, len(body)], np.uint64), r_t, n_t, m_t, a_t, s_t,
                                   chain_id=1, signer_kind=M.SIGNER_EIP155, max_txs=max_txs)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (r_t, n_t, m_t, a_t, s_t))


def _oracle_verdict(oracle, blob, cid, signer):
    st, addr = oracle.tx_sender(blob, cid, signer)
    return st, (addr.hex() if addr else None)


def _report(bad, n=4):
    return "%d disagreements; first %d:\n" % (len(bad), min(n, len(bad))) + "\n".join(
        "%s\n  blob %s\n  model %s\n  oracle %s\n  gpu %s" % b for b in bad[:n])


def _compare(oracle, cases, exp, status, senders, cid, signer, bad):
    """status and sender per case (zero address where the status is not ST_OK)"""
    for k, (c, (st, addr, d)) in enumerate(zip(cases, exp)):
        want = addr if st == M.ST_OK else bytes(20)
        if int(status[k]) != st or bytes(senders[k]) != want:
            bad.append(("%s (chain id %d, signer %d)" % (c.label, cid, signer), c.blob.hex(),
                        (st, addr.hex() if addr else d.get("error")), _oracle_verdict(oracle, c.blob, cid, signer),
                        (int(status[k]), bytes(senders[k]).hex())))


def _coverage(oracle, cov):
    """every status occurs, and every positive case is ST_OK with the signing key's address"""
    seen, addr = set(), C.key_address(oracle)
    for cases, exp, signer in cov:
        seen |= {e[0] for e in exp}
        pos = [(c, e) for c, e in zip(cases, exp) if C.positive_ok(c, signer)]
        assert len(pos) >= 20
        for c, e in pos:
            assert e[0] == M.ST_OK and e[1] == addr, (c.label, e[0])
    assert seen >= C.ALL_STATUSES, seen


@pytest.mark.parametrize("chain_id", C.CHAIN_IDS)
def test_notary_matches_model_on_corpus(ctx, oracle, corpora, chain_id):
    """ntx, status, sender and bitmap of every case under the three signers; chunk roots against the
    oracle's trie."""
    cases, bodies, roots_want = corpora[chain_id]
    bad, cov = [], []
    for signer in C.SIGNERS:
        exp = C.expected(oracle, cases, chain_id, signer)
        cov.append((cases, exp, signer))
        roots, ntx, bitmap, senders, status = ctx.notary_validate_shards(bodies, chain_id, signer, PER_SHARD)
        for i in range(len(bodies)):
            lo = i * PER_SHARD
            n = len(cases[lo:lo + PER_SHARD])
            assert ntx[i] == n, (i, ntx[i], n)
            _compare(oracle, cases[lo:lo + n], exp[lo:lo + n], status[i], senders[i], chain_id, signer, bad)
            bm = np.zeros(PER_SHARD // 8, np.uint8)
            for t in range(n):
                if exp[lo + t][0] == M.ST_OK:
                    bm[t // 8] |= 1 << (t % 8)
            if not bad:
                assert (bitmap[i] == bm).all(), (i, signer)
            assert bytes(roots[i]) == roots_want[i], i
    assert not bad, _report(bad)
    _coverage(oracle, cov)


@pytest.mark.parametrize("chain_id", C.CHAIN_IDS)
def test_tx_sender_batch_matches_model_on_corpus(ctx, oracle, corpora, chain_id):
    cases = corpora[chain_id][0]
    blobs = [c.blob for c in cases]
    bad, cov = [], []
    for signer in C.SIGNERS:
        exp = C.expected(oracle, cases, chain_id, signer)
        cov.append((cases, exp, signer))
        addr, st = ctx.tx_sender_batch(blobs, chain_id, signer)
        _compare(oracle, cases, exp, st, addr, chain_id, signer, bad)
    assert not bad, _report(bad)
    _coverage(oracle, cov)


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_blob_index_against_model_deserialize(ctx, oracle, seed):
    """A body of 40-70 KiB (more than 1,024 chunks, so each k_blob_index thread owns a run of two or three
    chunks): blobs of 1 to 40 chunks, garbage, one blob longer than three threads' runs, terminal lengths
    1 and 31, indicator bits 5 and 6 set, skipEvm, a terminal chunk first, non-terminal chunks last, a
    length that is no multiple of 32, and a max_txs that cuts the body off mid-way.  The blob boundaries
    come from the model's Deserialize; statuses and senders show whether a boundary moved."""
    from gsv._lib import GsvError
    body, max_txs = C.index_body(oracle, seed)
    blobs = M.deserialize(body)
    assert 1024 < len(body) // 32 <= 3 * 1024 and len(body) % 32 and 8 <= max_txs < len(blobs)
    assert any(len(b) > 31 * 9 for b, _ in blobs) and any(s for _, s in blobs)
    assert {len(b) % 31 for b, _ in blobs} >= {0, 1}
    cases = [C.Case(b, "blob %d of the seed-%d body" % (t, seed)) for t, (b, _) in enumerate(blobs)]
    bad = []
    for mt in (max_txs, (len(blobs) + 63) & ~63):  # cut off mid-way, and whole
        k = min(mt, len(blobs))
        exp = C.expected(oracle, cases[:k], 1, M.SIGNER_EIP155)
        if mt >= len(blobs):
            roots, ntx, bitmap, senders, status = ctx.notary_validate_shards([body], 1, M.SIGNER_EIP155, mt)
        else:
            # more blobs than max_txs: the host entry point refuses the shard (gsv.h: GSV_E_TOO_LARGE);
            # the device-resident one validates the first max_txs and reports the whole count in ntx
            with pytest.raises(GsvError) as e:
                ctx.notary_validate_shards([body], 1, M.SIGNER_EIP155, mt)
            assert e.value.code == -5
            roots, ntx, bitmap, senders, status = _validate_dev(ctx, body, mt)
        assert ntx[0] == len(blobs), (ntx[0], len(blobs))
        _compare(oracle, cases[:k], exp, status[0], senders[0], 1, M.SIGNER_EIP155, bad)
        bm = np.zeros((mt + 7) // 8, np.uint8)
        for t in range(k):
            if exp[t][0] == M.ST_OK:
                bm[t // 8] |= 1 << (t % 8)
        if not bad:
            assert (bitmap[0] == bm).all(), mt
        assert bytes(roots[0]) == oracle.derive_sha_bytes(body)
        assert {e[0] for e in exp} >= C.ALL_STATUSES
    assert not bad, _report(bad)
