"""GPU parity of proposer.createCollation as one call (csrc/gsv_proposer.hip: the serialize kernel, the
chunk roots of the bodies it wrote, the unsigned header hash, crypto.Sign) with the oracle-derived
fixture tests/golden/proposer_small.json, byte for byte, through the host form, the device-resident form
and sharding.CreateCollations; then the loop closed: what the proposer call builds, the notary call
validates."""
import hashlib

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

N_ORDER = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
GUARD = 0xEE


def be32(x):
    return int(x).to_bytes(32, "big")


def rows(bs, width):
    return np.frombuffer(b"".join(bs), np.uint8).reshape(-1, width).copy()


@pytest.fixture(scope="module")
def fx():
    g = golden("proposer_small.json")["collations"]
    return {
        "g": g,
        "txs": [[bytes.fromhex(t) for t in c["txs"]] for c in g],
        "sid": rows([be32(c["shard_id"]) for c in g], 32),
        "per": rows([be32(c["period"]) for c in g], 32),
        "prop": rows([bytes.fromhex(c["proposer"]) for c in g], 20),
        "key": rows([bytes.fromhex(c["key"]) for c in g], 32),
    }


def check_golden(g, bodies, root, h, sig, st, idx=None):
    for j, c in enumerate(g):
        i = j if idx is None else idx[j]
        assert st[i] == 0, c["name"]
        assert len(bodies[i]) == c["body_len"] and hashlib.sha256(bodies[i]).hexdigest() == c["body_sha256"], c["name"]
        assert bytes(root[i]).hex() == c["chunk_root"], c["name"]
        assert bytes(h[i]).hex() == c["hash"], c["name"]
        assert bytes(sig[i]).hex() == c["sig"], c["name"]


def dev_run(ctx, tx_lists, sid, per, prop, key, stream=None, graph=False):
    """the _dev form on an explicit stream, outputs over-allocated by a guard row / guard bytes"""
    import torch
    import gsv
    from gsv import _blob_tables
    dev = torch.device("cuda", ctx.device)
    n = len(tx_lists)
    flat, bo, lo = _blob_tables(tx_lists)
    body_off, _ = gsv.proposer_body_layout(bo, lo)
    total = int(body_off[-1])
    to = lambda a: torch.from_numpy(np.array(a)).to(dev)  # noqa: E731
    d_blobs, d_sid, d_per, d_prop, d_key = to(flat), to(sid), to(per), to(prop), to(key)
    outs = [torch.full(s, GUARD, dtype=torch.uint8, device=dev)
            for s in ((total + 256,), (n + 1, 32), (n + 1, 32), (n + 1, 65), (n + 1,))]
    cs = stream or torch.cuda.Stream(device=dev)
    ctx.proposer_prepare(bo, lo)
    torch.cuda.synchronize()

    def call():
        ctx.proposer_create_collations_dev(d_blobs, bo, lo, d_sid, d_per, d_prop, d_key, *outs, stream=cs,
                                           prepare=False)
    if graph:
        call()  # warm, uncaptured
        cs.synchronize()
        plain = [o.clone() for o in outs]
        g = torch.cuda.CUDAGraph()
        shapes_before = ctx.prepared_shapes()
        with torch.cuda.graph(g, stream=cs):
            call()
        assert ctx.prepared_shapes() == shapes_before  # nothing allocated inside the capture
        for o in outs:
            o.fill_(GUARD)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(plain, outs):
            assert torch.equal(a, b)
    else:
        call()
        cs.synchronize()
    b, root, h, sig, st = (o.cpu().numpy() for o in outs)
    assert (b[total:] == GUARD).all() and (root[n] == GUARD).all() and (h[n] == GUARD).all()
    assert (sig[n] == GUARD).all() and st[n] == GUARD
    bodies = [b[int(body_off[i]):int(body_off[i + 1])].tobytes() for i in range(n)]
    return bodies, root, h, sig, st


def test_golden_host_form(ctx, fx):
    out = ctx.proposer_create_collations(fx["txs"], fx["sid"], fx["per"], fx["prop"], fx["key"])
    check_golden(fx["g"], *out)


def test_golden_dev_form(ctx, fx):
    out = dev_run(ctx, fx["txs"], fx["sid"], fx["per"], fx["prop"], fx["key"])
    check_golden(fx["g"], *out)


def test_golden_create_collations(ctx, fx):
    from gsv import sharding
    g = fx["g"]
    cols = sharding.CreateCollations(fx["txs"], [c["shard_id"] for c in g], [c["period"] for c in g],
                                     [bytes.fromhex(c["proposer"]) for c in g], [int(c["key"], 16) for c in g], ctx)
    assert len(cols) == len(g)
    for col, c in zip(cols, g):
        hd = col.Header()
        assert hashlib.sha256(col.Body()).hexdigest() == c["body_sha256"]
        assert hd.ChunkRoot().hex() == c["chunk_root"] and hd.Sig().hex() == c["sig"]
        assert hd.ShardID() == c["shard_id"] and hd.Period() == c["period"] and hd.ProposerAddress().hex() == c["proposer"]
        assert col.transactions == [bytes.fromhex(t) for t in c["txs"]]
    assert [bytes(x).hex() for x in sharding.HeaderHashBatch([col.Header() for col in cols], ctx)] == \
        [c["signed_hash"] for c in g]
    assert sharding.CreateCollations([], [], [], [], [], ctx) == []


@pytest.fixture(scope="module")
def mixed(fx):
    """valid | oversized (32,769 chunks) | key 0 | key >= n | valid"""
    big = [bytes([1 + i % 250]) * 124 for i in range(8192)] + [b"\x01"]
    order = [0, None, 1, 0, 2]  # the fixture collation behind each slot
    txs = [fx["txs"][0], big, fx["txs"][1], fx["txs"][0], fx["txs"][2]]
    sid = fx["sid"][[0, 1, 1, 0, 2]]
    per = fx["per"][[0, 1, 1, 0, 2]]
    prop = fx["prop"][[0, 1, 1, 0, 2]]
    key = fx["key"][[0, 1, 1, 0, 2]].copy()
    key[2] = 0
    key[3] = np.frombuffer(be32(N_ORDER), np.uint8)
    return txs, sid, per, prop, key


def check_mixed(fx, out):
    from gsv import _lib
    g = fx["g"]
    bodies, root, h, sig, st = out
    assert list(st[:5]) == [_lib.ST_OK, _lib.ST_BODY_TOO_LARGE, _lib.ST_INVALID_KEY, _lib.ST_INVALID_KEY, _lib.ST_OK]
    check_golden([g[0], g[2]], bodies, root, h, sig, st, idx=[0, 4])  # the neighbours are unaffected
    assert bodies[1] == b"" and not root[1].any() and not h[1].any() and not sig[1].any()
    for i, c in ((2, g[1]), (3, g[0])):  # an invalid key: no signature, everything else as the fixture
        assert hashlib.sha256(bodies[i]).hexdigest() == c["body_sha256"]
        assert bytes(root[i]).hex() == c["chunk_root"] and bytes(h[i]).hex() == c["hash"]
        assert not sig[i].any()


def test_mixed_batch_host_form(ctx, fx, mixed):
    check_mixed(fx, ctx.proposer_create_collations(*mixed))


def test_mixed_batch_dev_form(ctx, fx, mixed):
    check_mixed(fx, dev_run(ctx, *mixed))


def test_create_collations_raises(ctx, fx, mixed):
    from gsv import crypto, sharding
    g = fx["g"]
    txs = mixed[0]
    args = lambda idx: ([g[i]["shard_id"] for i in idx], [g[i]["period"] for i in idx],  # noqa: E731
                        [bytes.fromhex(g[i]["proposer"]) for i in idx])
    with pytest.raises(ValueError, match="the serialized body size 1048608 exceeded the collation size limit 1048576"):
        sharding.CreateCollations([txs[0], txs[1]], *args([0, 1]), [int(g[0]["key"], 16), int(g[1]["key"], 16)], ctx)
    for bad in (0, N_ORDER):
        with pytest.raises(crypto.ErrInvalidKey, match="invalid private key"):
            sharding.CreateCollations([txs[0], txs[2]], *args([0, 1]), [int(g[0]["key"], 16), bad], ctx)


def test_the_notary_validates_what_the_proposer_builds(ctx, fx):
    from gsv import sharding
    g = fx["g"]
    cols = sharding.CreateCollations(fx["txs"], [c["shard_id"] for c in g], [c["period"] for c in g],
                                     [bytes.fromhex(c["proposer"]) for c in g], [int(c["key"], 16) for c in g], ctx)
    roots, ntx, bitmap, senders, status = ctx.notary_validate_shards([c.Body() for c in cols], 1, 0, 16)
    for i, (col, c) in enumerate(zip(cols, g)):
        assert bytes(roots[i]) == col.Header().ChunkRoot()
        assert ntx[i] == len(c["txs"])
        assert (status[i, :ntx[i]] == 0).all()
        assert [bytes(senders[i, t]).hex() for t in range(ntx[i])] == c["senders"]
    signer, st = sharding.VerifyProposerSignatures([col.Header() for col in cols], ctx)
    assert (st == 0).all()
    assert [bytes(s).hex() for s in signer] == [c["proposer"] for c in g]


def test_dev_form_is_capturable(ctx, fx):
    """captured once on a gsv_stream_create stream, replayed once: the uncaptured run's outputs"""
    (cs,) = ctx.pipeline_streams(1)
    try:
        out = dev_run(ctx, fx["txs"], fx["sid"], fx["per"], fx["prop"], fx["key"], stream=cs, graph=True)
        check_golden(fx["g"], *out)
    finally:
        ctx.destroy_streams([cs])


def test_unprepared_and_misaligned(ctx):
    import torch
    from gsv import GsvError, _lib
    dev = torch.device("cuda", ctx.device)
    bo = np.array([0, 45, 2345], np.uint64)  # offsets no other test prepares
    lo = np.array([0, 1, 2], np.uint64)
    t = torch.zeros((4096,), dtype=torch.uint8, device=dev)
    with pytest.raises(GsvError) as e:
        ctx.proposer_create_collations_dev(t, bo, lo, t, t, t, t, t, t, t, t, t, prepare=False)
    assert e.value.code == _lib.E_NOT_PREPARED
    ctx.proposer_prepare(bo, lo)
    with pytest.raises(GsvError) as e:
        ctx.proposer_create_collations_dev(t, bo, lo, t, t, t, t, t[8:], t, t, t, t, prepare=False)
    assert e.value.code == _lib.E_INVALID_ARG


def test_staged_keys_are_wiped(ctx, fx):
    """after the host form returns, the arena's key region (the first: offset 0, 32 n bytes) holds none
    of the key bytes; the region behind it still holds the transactions this call staged"""
    n = 40
    txs = [[bytes([0x3C]) * 100] for _ in range(n)]
    keys = np.full((n, 32), 0xA5, np.uint8)
    sid = np.zeros((n, 32), np.uint8)
    prop = np.zeros((n, 20), np.uint8)
    bodies, root, h, sig, st = ctx.proposer_create_collations(txs, sid, sid, prop, keys)
    assert (st == 0).all() and sig.any()
    assert not ctx._arena_read(0, n * 32).any(), "staged secret keys left in the arena"
    behind = (n * 32 + 255) // 256 * 256
    assert (ctx._arena_read(behind, n * 100) == 0x3C).all()
