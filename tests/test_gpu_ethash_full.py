"""GPU tests of the sealing half of the ethash family (include/gsv.h): the device-resident dataset, hashimotoFull,
VerifySeal over the dataset, the nonce search and Seal.  Expected values come from the recorded results of the
reference's libethash (tests/golden/ethash.json) and the numpy model (tests/ethash_model.py, pinned to that
fixture by tests/test_ethash_cpu.py), never from the library."""
import numpy as np
import pytest

import ethash_model as M
from conftest import golden

pytestmark = pytest.mark.gpu

GUARD = 0xEE
TEST_DATASET = 32 * 1024
MAXU = (1 << 256) - 1
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def fx():
    return golden("ethash.json")


def _rows(rows):
    h = np.frombuffer(bytes.fromhex("".join(r["hash"] for r in rows)), np.uint8).reshape(-1, 32)
    n = np.array([r["nonce"] for r in rows], np.uint64)
    mix = np.frombuffer(bytes.fromhex("".join(r["mix"] for r in rows)), np.uint8).reshape(-1, 32)
    res = np.frombuffer(bytes.fromhex("".join(r["result"] for r in rows)), np.uint8).reshape(-1, 32)
    return h, n, mix, res


def _dev(ctx, a):
    import torch
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(torch.device("cuda", ctx.device))


def _series(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(0, 2**64, n, dtype=np.uint64)


def _be32(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "big") for v in values), np.uint8).reshape(-1, 32)


def _ints(rows):
    return [int.from_bytes(x.tobytes(), "big") for x in rows]


@pytest.fixture(scope="module")
def small(ctx, fx):
    """the test-mode shape: the 1 KiB cache, the model's 32 KiB dataset (512 items, 256 pages) and the library's
    dataset on the device"""
    from gsv import ethash as E
    raw = np.frombuffer(bytes.fromhex(fx["test_mode"]["cache0"]), np.uint8)
    dataset = M.dataset_item(M.words(raw), np.arange(512, dtype=np.uint32))
    return raw, dataset, E.generateDataset(TEST_DATASET, raw, ctx)


@pytest.fixture(scope="module")
def series1000(small):
    h, n = _series(1000, 0xE7A5)
    d, r = M.hashimoto_full(TEST_DATASET, small[1], h, n)
    return h, n, d, r


# ---------------------------------------------------------------- 1. the dataset
def test_generate_dataset_test_mode(ctx, fx, small):
    _, dataset, d_set = small
    assert d_set.is_cuda and d_set.numel() == TEST_DATASET and d_set.data_ptr() % 128 == 0
    got = d_set.cpu().numpy()
    assert got.tobytes() == M.item_bytes(dataset)
    assert M.keccak256_bytes(got.tobytes()).hex() == fx["test_mode"]["dataset_digest"]


# ---------------------------------------------------------------- 2. hashimotoFull
def test_full_go_vector_and_fixture_rows(ctx, fx, small):
    from gsv import ethash as E
    d_set = small[2]
    go = fx["test_mode"]["go"]
    digest, result = E.hashimotoFull(d_set, bytes.fromhex(go["hash"]), go["nonce"], ctx)
    assert digest.hex() == go["digest"] and result.hex() == go["result"]
    h, n, mix, res = _rows(fx["test_mode"]["light"])
    d, r = E.hashimotoFullBatch(d_set, h, n, ctx)
    assert (d == mix).all() and (r == res).all()


@pytest.mark.parametrize("n", [0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 257, 1000])
def test_full_matches_model_at_group_and_wave_edges(ctx, small, series1000, n):
    """partial groups of eight, partial waves, a group straddling the batch's end, more than one workgroup"""
    from gsv import ethash as E
    h, nn, want_d, want_r = series1000
    d, r = E.hashimotoFullBatch(small[2], h[:n], nn[:n], ctx)
    assert d.shape == (n, 32) and (d == want_d[:n]).all() and (r == want_r[:n]).all()


# ---------------------------------------------------------------- 3. verify over the dataset
def test_verify_seal_full_statuses(ctx, small, series1000):
    import torch
    from gsv import _lib
    d_set = small[2]
    h, nn, mix, res = (a[:64] for a in series1000)
    r = _ints(res)
    assert all(v > 1 for v in r)
    d_h, d_n = _dev(ctx, h), _dev(ctx, nn)

    def run(mixes, diffs):
        st = torch.full((64,), GUARD, dtype=torch.uint8, device=d_h.device)
        d_mix, d_diff = _dev(ctx, mixes), _dev(ctx, _be32(diffs))
        ctx.ethash_verify_seal_full_batch_dev(d_set, d_h, d_n, d_mix, d_diff, st)
        torch.cuda.synchronize()
        return st.cpu().numpy()

    assert (run(mix, [MAXU // v for v in r]) == _lib.ST_OK).all()
    assert (run(mix, [MAXU // v + 1 for v in r]) == _lib.ST_INVALID_POW).all()
    assert (run(mix, [1] * 64) == _lib.ST_OK).all()
    assert (run(mix, [MAXU] * 64) == _lib.ST_INVALID_POW).all()  # target 1, every r above it
    bad = mix.copy()
    bad[np.arange(64), np.arange(64) % 32] ^= np.uint8(1) << (np.arange(64) % 8).astype(np.uint8)
    assert (run(bad, [0] * 64) == _lib.ST_INVALID_DIFFICULTY).all()  # even with a wrong mix
    assert (run(mix, [0] * 64) == _lib.ST_INVALID_DIFFICULTY).all()
    assert (run(bad, [MAXU // v + 1 for v in r]) == _lib.ST_INVALID_MIX_DIGEST).all()  # even where the PoW fails too
    assert (run(bad, [1] * 64) == _lib.ST_INVALID_MIX_DIGEST).all()
    diffs = [MAXU // v + (k % 2) for k, v in enumerate(r)]
    want = np.array([_lib.ST_INVALID_POW if k % 2 else _lib.ST_OK for k in range(64)], np.uint8)
    assert (run(mix, diffs) == want).all()


# ---------------------------------------------------------------- 4. the search, device form
SPAN = 8192


@pytest.fixture(scope="module")
def headers():
    rng = np.random.default_rng(0x5EA1)
    H = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    S = rng.integers(0, 2**63, 8, dtype=np.uint64)
    return H, S


def _model_span(dataset, h, start, span):
    """the model over nonces start .. start + span - 1 (mod 2^64) of one header: digests, results, results as ints"""
    nonces = np.uint64(start) + np.arange(span, dtype=np.uint64)  # wraps
    d, r = M.hashimoto_full(TEST_DATASET, dataset, np.tile(h, (span, 1)), nonces)
    return nonces, d, r, _ints(r)


@pytest.fixture(scope="module")
def model8(small, headers):
    """the model's hashimotoFull over the first 8,192 nonces of each of the 8 headers, computed once"""
    H, S = headers
    return [_model_span(small[1], H[k], S[k], SPAN) for k in range(8)]


def _first(ints, difficulty, span):
    """offset of the first winner among the first `span` results, or None"""
    if difficulty == 0:
        return None
    target = MAXU // difficulty
    return next((k for k in range(span) if ints[k] <= target), None)


def _search(ctx, d_set, H, diffs, S, span):
    import torch
    dev = d_set.device
    n = len(S)
    d_h, d_s = _dev(ctx, H), _dev(ctx, np.asarray(S, np.uint64))
    d_d = _dev(ctx, diffs if isinstance(diffs, np.ndarray) else _be32(diffs))
    off = torch.zeros(n, dtype=torch.int32, device=dev)
    non = torch.full((n,), -1, dtype=torch.int64, device=dev)
    mix = torch.full((n, 32), GUARD, dtype=torch.uint8, device=dev)
    res = torch.full((n, 32), GUARD, dtype=torch.uint8, device=dev)
    fnd = torch.full((n,), GUARD, dtype=torch.uint8, device=dev)
    ctx.ethash_search_dev(d_set, d_h, d_d, d_s, span, off, non, mix, res, fnd)
    torch.cuda.synchronize()
    return (off.cpu().numpy().view(np.uint32), non.cpu().numpy().view(np.uint64), mix.cpu().numpy(),
            res.cpu().numpy(), fnd.cpu().numpy())


def _check_search(got, model, diffs, span):
    off, non, mix, res, fnd = got
    for k, (nonces, d, r, ints) in enumerate(model):
        w = _first(ints, diffs[k], span)
        if w is None:
            assert fnd[k] == 0 and off[k] == NONE and non[k] == 0 and not mix[k].any() and not res[k].any(), k
        else:
            assert fnd[k] == 1 and off[k] == w and non[k] == nonces[w], (k, off[k], w)
            assert (mix[k] == d[w]).all() and (res[k] == r[w]).all(), k
    return [_first(m[3], diffs[k], span) for k, m in enumerate(model)]


def test_search_smallest_winner(ctx, small, headers, model8):
    H, S = headers
    # every header has several winners in the span, so the smallest-winner rule is exercised
    for k in range(8):
        target = MAXU // 1024
        assert sum(v <= target for v in model8[k][3]) >= 2
    firsts = _check_search(_search(ctx, small[2], H, [1024] * 8, S, SPAN), model8, [1024] * 8, SPAN)
    assert all(w is not None and w >= 64 for w in firsts)
    # none of them inside the first 64 nonces
    assert _check_search(_search(ctx, small[2], H, [1024] * 8, S, 64), model8, [1024] * 8, 64) == [None] * 8
    firsts = _check_search(_search(ctx, small[2], H, [64] * 8, S, 512), model8, [64] * 8, 512)
    assert all(w is not None for w in firsts)


def test_search_mixed_difficulties(ctx, small, headers, model8):
    H, S = headers
    diffs = [1, 64, 1024, 0, MAXU, 1, 0, 1024]
    firsts = _check_search(_search(ctx, small[2], H, diffs, S, 512), model8, diffs, 512)
    assert firsts[0] == 0 and firsts[5] == 0  # difficulty 1: the first nonce wins
    assert firsts[3] is None and firsts[6] is None  # difficulty 0 never wins
    assert firsts[4] is None  # target 1


def test_search_wraps_past_2_64(ctx, small, headers):
    H, _ = headers
    start = 2**64 - 5
    model = [_model_span(small[1], H[0], start, 64)]
    assert int(model[0][0][5]) == 0  # the sixth nonce is 0
    got = _search(ctx, small[2], H[:1], [1], [start], 64)
    assert _check_search(got, model, [1], 64) == [0] and got[1][0] == start
    # a difficulty whose first winner is the smallest result behind the wrap
    ints = model[0][3]
    w = min(range(5, 64), key=lambda k: ints[k])
    diff = MAXU // ints[w]
    assert _first(ints, diff, 64) == w  # the model's first winner lies past the wrap
    got = _search(ctx, small[2], H[:1], [diff], [start], 64)
    assert _check_search(got, model, [diff], 64) == [w] and got[1][0] == (start + w) % 2**64


# ---------------------------------------------------------------- 5. Seal, host and Python forms
def test_seal_python(ctx, small, headers, model8):
    from gsv import ethash as E
    H, S = headers
    eng = E.Ethash(test_mode=True, ctx=ctx)  # block 0 in test mode: the fixture's cache and dataset
    nonces, d, r, ints = model8[0]
    w = _first(ints, 1024, SPAN)
    assert w is not None and w > 0
    h, start = H[0].tobytes(), int(S[0])
    got = eng.Seal(0, h, 1024, start, max_attempts=SPAN)
    assert got == (int(nonces[w]), d[w].tobytes())
    eng.VerifySeal(0, h, got[0], got[1], 1024)
    assert eng.Seal(0, h, 1024, start, max_attempts=w) is None  # one short of the winner
    assert eng.Seal(0, h, 1024, start, max_attempts=w + 1) == got
    with pytest.raises(E.ErrInvalidDifficulty):
        eng.Seal(0, h, 0, start, max_attempts=16)
    assert eng.Seal(0, h, 1 << 256, start, max_attempts=512) is None  # target 0
    # the by-number hashimotoFull over the context's dataset
    dd, rr = eng.hashimotoFull([0, 29999], [h, h], [int(nonces[w]), int(nonces[0])])
    assert (dd[0] == d[w]).all() and (rr[0] == r[w]).all() and (dd[1] == d[0]).all() and (rr[1] == r[0]).all()


def test_seal_batch_across_epochs(ctx, headers):
    from gsv import _lib
    from gsv import ethash as E
    H, S = headers
    epochs = [0, 1, 2]
    numbers = np.array([epochs[k % 3] * 30000 + 11 * k for k in range(8)], np.uint64)
    diffs = [64, 64, 64, 1024, 1024, 0, 1024, 2**40]
    eng = E.Ethash(test_mode=True, ctx=ctx)
    nonce, mix, st = eng.SealBatch(numbers, H, diffs, S, 2048)
    assert ctx.ethash_datasets() == _lib.ETHASH_MAX_DATASETS == 2
    for k in range(8):
        cache = E.generateCache(1024, E.seedHash(epochs[k % 3] * 30000))
        dataset = M.dataset_item(M.words(cache), np.arange(512, dtype=np.uint32))
        nonces, d, r, ints = _model_span(dataset, H[k], S[k], 2048)
        w = _first(ints, diffs[k], 2048)
        if diffs[k] == 0:
            assert st[k] == _lib.ST_INVALID_DIFFICULTY and nonce[k] == 0 and not mix[k].any()
        elif w is None:
            assert st[k] == _lib.ST_NONCE_NOT_FOUND and nonce[k] == 0 and not mix[k].any()
        else:
            assert st[k] == _lib.ST_OK and nonce[k] == nonces[w] and (mix[k] == d[w]).all(), k
    assert (st == _lib.ST_OK).sum() >= 4 and st[7] == _lib.ST_NONCE_NOT_FOUND


def test_seal_in_several_rounds(ctx, small):
    """16,384 headers take rounds of 256 nonces each (csrc/ethash_host.h seal_round), so 1,024 attempts are four
    rounds and the found headers leave in between.  The first 24 headers are checked against the model, first
    winners in later rounds among them; all of them against ONE search launch over 1,024 nonces, which the
    tests above pin to the model."""
    from gsv import _lib
    from gsv import ethash as E
    m = 16384
    H, S = _series(m, 0x5EA2)
    diffs = _be32([256]).repeat(m, axis=0)
    nonce, mix, st = E.Ethash(test_mode=True, ctx=ctx).SealBatch(np.zeros(m, np.uint64), H, diffs, S, 1024)
    rounds = set()
    for k in range(24):
        nonces, d, r, ints = _model_span(small[1], H[k], S[k], 1024)
        w = _first(ints, 256, 1024)
        if w is None:
            assert st[k] == _lib.ST_NONCE_NOT_FOUND and nonce[k] == 0 and not mix[k].any(), k
        else:
            rounds.add(w // 256)
            assert st[k] == _lib.ST_OK and nonce[k] == nonces[w] and (mix[k] == d[w]).all(), k
    assert len(rounds) >= 2
    off, non, dmix, _, fnd = _search(ctx, small[2], H, diffs, S, 1024)
    assert ((st == _lib.ST_OK) == (fnd == 1)).all() and (nonce == non).all() and (mix == dmix).all()
    assert 0 < (fnd == 0).sum() < m // 8  # (1 - 1/256)^1024 = 1.8 % stay unfound


# ---------------------------------------------------------------- 6. the _dev contract
def test_dev_form_contract(ctx, small, series1000, headers, model8):
    import torch
    from gsv import GsvError, _lib
    _, dataset, d_set = small
    dev = d_set.device
    n = 65
    h, nn, want_d, want_r = (a[:n] for a in series1000)
    hbuf = torch.zeros(4 + 32 * n, dtype=torch.uint8, device=dev)
    nbuf = torch.zeros(8 + 8 * n, dtype=torch.uint8, device=dev)
    d_h, d_n = hbuf[4:], nbuf[8:]
    assert d_h.data_ptr() % 16 == 4 and d_n.data_ptr() % 16 == 8
    d_h.copy_(_dev(ctx, h).reshape(-1))
    d_n.copy_(_dev(ctx, nn.view(np.uint8)))
    mbuf = torch.full((64 + 32 * n,), GUARD, dtype=torch.uint8, device=dev)
    rbuf = torch.full((64 + 32 * n,), GUARD, dtype=torch.uint8, device=dev)
    d_mix, d_res = mbuf[17:17 + 32 * n], rbuf[3:3 + 32 * n]
    torch.cuda.synchronize()
    cs = torch.cuda.Stream()

    def check(wd, wr, rows=n):
        m, r = mbuf.cpu().numpy(), rbuf.cpu().numpy()
        assert (m[17:17 + 32 * rows].reshape(rows, 32) == wd).all() and (r[3:3 + 32 * rows].reshape(rows, 32) == wr).all()
        assert (m[:17] == GUARD).all() and (m[17 + 32 * rows:] == GUARD).all()
        assert (r[:3] == GUARD).all() and (r[3 + 32 * rows:] == GUARD).all()

    # the search's buffers: 8 headers, found bytes at an odd offset
    H, S = headers
    s_h, s_d, s_s = _dev(ctx, H), _dev(ctx, _be32([1024] * 8)), _dev(ctx, S)
    obuf = torch.zeros(4 + 4 * 8, dtype=torch.uint8, device=dev)
    s_off = obuf[4:]
    s_non = torch.zeros(8, dtype=torch.int64, device=dev)
    fbuf = torch.full((32,), GUARD, dtype=torch.uint8, device=dev)
    s_fnd = fbuf[5:13]

    def search(span=SPAN, stream=cs, **k):
        a = dict(dataset_t=d_set, hash_t=s_h, difficulty_t=s_d, start_t=s_s, span=span, offset_t=s_off, nonce_out_t=s_non,
                 mix_t=d_mix, result_t=d_res, found_t=s_fnd, stream=stream, n=8)
        a.update(k)
        ctx.ethash_search_dev(**a)

    def check_search(model, span=SPAN):
        f = fbuf.cpu().numpy()
        assert (f[:5] == GUARD).all() and (f[13:] == GUARD).all() and (f[5:13] == 1).all()
        w = [_first(m[3], 1024, span) for m in model]
        assert (obuf.cpu().numpy()[4:].view(np.uint32) == np.array(w, np.uint32)).all()
        assert (s_non.cpu().numpy().view(np.uint64) == np.array([m[0][k] for m, k in zip(model, w)], np.uint64)).all()
        check(np.stack([m[1][k] for m, k in zip(model, w)]), np.stack([m[2][k] for m, k in zip(model, w)]), rows=8)

    ctx.set_timing(True)
    try:
        ctx.reset_timing()
        ctx.ethash_full_batch_dev(d_set, d_h, d_n, d_mix, d_res, stream=cs, n=n)
        cs.synchronize()
        check(want_d, want_r)
        mbuf.fill_(GUARD)
        rbuf.fill_(GUARD)
        torch.cuda.synchronize()
        search()
        cs.synchronize()
        for kid in (_lib.K_ETHASH_FULL, _lib.K_ETHASH_SEARCH, _lib.K_ETHASH_FINISH):
            ms, launches = ctx.kernel_time(kid)
            assert launches == 1 and ms > 0, kid
        # n == 0 enqueues nothing: no launch is counted under any of the three ids
        ctx.ethash_full_batch_dev(d_set, None, None, None, None, stream=cs, n=0)
        ctx.ethash_verify_seal_full_batch_dev(d_set, None, None, None, None, None, stream=cs, n=0)
        search(hash_t=None, difficulty_t=None, start_t=None, offset_t=None, nonce_out_t=None, mix_t=None,
               result_t=None, found_t=None, n=0)
        cs.synchronize()
        for kid in (_lib.K_ETHASH_FULL, _lib.K_ETHASH_SEARCH, _lib.K_ETHASH_FINISH):
            assert ctx.kernel_time(kid)[1] == 1, kid
    finally:
        ctx.set_timing(False)
        ctx.reset_timing()
    check_search(model8)

    def refused(fn, *a, **k):
        with pytest.raises(GsvError) as e:
            fn(*a, **k)
        assert e.value.code == _lib.E_INVALID_ARG

    full = ctx.ethash_full_batch_dev
    refused(full, d_set, hbuf[2:], d_n, d_mix, d_res, n=n)  # a hash row off 4-byte alignment
    refused(full, d_set, d_h, nbuf[4:], d_mix, d_res, n=n)  # nonces off 8-byte alignment
    refused(full, d_set[64:64 + 128], d_h, d_n, d_mix, d_res, n=n)  # a dataset off 128-byte alignment
    for size in (0, 64, 128 + 64):
        refused(full, d_set[:size], d_h, d_n, d_mix, d_res, n=n)
    refused(ctx.ethash_verify_seal_full_batch_dev, d_set[16:16 + 128], d_h, d_n, d_mix, d_res, fbuf, n=8)
    refused(search, span=0)
    refused(search, span=1 << 32)
    refused(search, span=(1 << 32) - 1, n=129)  # 129 x 2^24 workgroups: past the grid (refused before any launch)
    refused(search, offset_t=obuf[2:])
    refused(search, start_t=nbuf[4:])
    refused(search, nonce_out_t=nbuf[4:])
    refused(search, dataset_t=d_set[64:64 + 128])
    full(d_set, None, None, None, None, n=0)  # n == 0: no launch
    search(hash_t=None, difficulty_t=None, start_t=None, offset_t=None, nonce_out_t=None, mix_t=None, result_t=None,
           found_t=None, n=0)
    torch.cuda.synchronize()
    check_search(model8)

    # captured on an explicit stream, replayed twice with changed nonces / starts
    before = (ctx.ethash_datasets(), ctx.ethash_caches())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        full(d_set, d_h, d_n, d_mix, d_res, stream=cs, n=n)
    gs = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gs, stream=cs):
        search(span=512)
    assert (ctx.ethash_datasets(), ctx.ethash_caches()) == before
    s_d.copy_(_dev(ctx, _be32([64] * 8)))
    for shift in (1, 2):
        nn2 = np.roll(nn, shift)
        wd, wr = M.hashimoto_full(TEST_DATASET, dataset, h, nn2)
        d_n.copy_(_dev(ctx, nn2.view(np.uint8)))
        mbuf.fill_(GUARD)
        rbuf.fill_(GUARD)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check(wd, wr)
        # the search from starts moved forward by `shift`: the model's rows from that offset on
        s_s.copy_(_dev(ctx, S + np.uint64(shift)))
        mbuf.fill_(GUARD)
        rbuf.fill_(GUARD)
        fbuf.fill_(GUARD)
        torch.cuda.synchronize()
        gs.replay()
        torch.cuda.synchronize()
        moved = [(m[0][shift:], m[1][shift:], m[2][shift:], m[3][shift:]) for m in model8]
        f = fbuf.cpu().numpy()
        w = [_first(m[3], 64, 512) for m in moved]
        assert all(k is not None for k in w) and (f[5:13] == 1).all() and (f[:5] == GUARD).all() and (f[13:] == GUARD).all()
        assert (obuf.cpu().numpy()[4:].view(np.uint32) == np.array(w, np.uint32)).all()
        check(np.stack([m[1][k] for m, k in zip(moved, w)]), np.stack([m[2][k] for m, k in zip(moved, w)]), rows=8)


# ---------------------------------------------------------------- 7. real row counts: epoch 0
def test_full_epoch0(ctx, fx):
    from gsv import ethash as E
    size = E.datasetSize(0)
    assert size == 1073739904
    d_set = E.generateDataset(size, E.generateCache(E.cacheSize(0), E.seedHash(0)), ctx)
    assert fx["items"][-1]["index"] == size // 64 - 1
    for r in fx["items"]:
        at = r["index"] * 64
        assert d_set[at:at + 64].cpu().numpy().tobytes().hex() == r["bytes"], r["index"]
    h, n, mix, res = _rows(fx["light"]["0"])
    assert len(n) == 16
    d, r = E.hashimotoFullBatch(d_set, h, n, ctx)
    assert (d == mix).all() and (r == res).all()
    del d_set
    numbers = np.array([29999 - 1873 * k for k in range(16)], np.uint64)
    d, r = E.Ethash(ctx=ctx).hashimotoFull(numbers, h, n)
    assert (d == mix).all() and (r == res).all()
    assert 1 <= ctx.ethash_datasets() <= 2


# ---------------------------------------------------------------- 8. byte offsets above 2^32
def _synthetic_words(j):
    """word j of the synthetic dataset, a closed form that numpy (uint64) and torch (int64) both evaluate:
    j < 2^31 and the multiplier < 2^32, so nothing passes 2^63"""
    return (j * 2654435761 + (j >> 9)) & 0xFFFFFFFF


def test_full_wide_offsets(ctx):
    """3 * 2^24 + 1 pages (6,442,451,072 bytes): a third of the accesses lie above 2^32 bytes, and the page count
    is no power of two"""
    import torch
    from gsv import ethash as E
    pages = 3 * (1 << 24) + 1
    size = pages * 128
    dev = torch.device("cuda", ctx.device)
    d_set = torch.empty(size // 4, dtype=torch.int32, device=dev)
    step = 1 << 24
    for first in range(0, size // 4, step):
        j = torch.arange(first, min(first + step, size // 4), dtype=torch.int64, device=dev)
        w = _synthetic_words(j)
        d_set[first:first + j.numel()] = torch.where(w >= 2**31, w - 2**32, w).to(torch.int32)
    assert d_set.data_ptr() % 128 == 0

    def lookup(idx):
        j = idx.astype(np.uint64).reshape(-1, 1) * np.uint64(16) + np.arange(16, dtype=np.uint64)
        return _synthetic_words(j).astype(np.uint32)

    probe = np.array([0, 1, size // 64 - 1], np.uint32)
    for k, row in zip(probe, lookup(probe)):
        assert (d_set[int(k) * 16:int(k) * 16 + 16].cpu().numpy().view(np.uint32) == row).all()
    h, n = _series(8, 0x77)
    want_d, want_r = M._hashimoto(size, h, n, lookup)
    d, r = E.hashimotoFullBatch(d_set.view(torch.uint8), h, n, ctx)
    assert (d == want_d).all() and (r == want_r).all()
