"""GPU tests of the ethash family (include/gsv.h): dataset items, hashimotoLight and VerifySeal against the
recorded results of the reference's libethash (tests/golden/ethash.json) and the numpy model
(tests/ethash_model.py, itself pinned to that fixture by tests/test_ethash_cpu.py)."""
import numpy as np
import pytest

import ethash_model as M
from conftest import golden

pytestmark = pytest.mark.gpu

GUARD = 0xEE
TEST_DATASET = 32 * 1024
MAXU = (1 << 256) - 1


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


@pytest.fixture(scope="module")
def small(ctx, fx):
    """the test-mode shape: the 1 KiB cache (host, device, words) and the model's 32 KiB dataset"""
    raw = np.frombuffer(bytes.fromhex(fx["test_mode"]["cache0"]), np.uint8)
    words = M.words(raw)
    dataset = M.dataset_item(words, np.arange(512, dtype=np.uint32))
    return raw, _dev(ctx, raw), words, dataset


@pytest.fixture(scope="module")
def full(ctx):
    """the epoch-0 and epoch-1 caches, made once by gsv_ethash_make_cache, on the device"""
    from gsv import ethash as E
    out = {}
    for block in (0, 30000):
        out[block] = (_dev(ctx, E.generateCache(E.cacheSize(block), E.seedHash(block))), E.datasetSize(block))
    return out


def _series(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(0, 2**64, n, dtype=np.uint64)


# ---------------------------------------------------------------- the test-mode shape
def test_go_vector_and_fixture_rows(ctx, fx, small):
    from gsv import ethash as E
    _, d_cache, _, _ = small
    go = fx["test_mode"]["go"]
    digest, result = E.hashimotoLight(TEST_DATASET, d_cache, bytes.fromhex(go["hash"]), go["nonce"], ctx)
    assert digest.hex() == go["digest"] and result.hex() == go["result"]
    h, n, mix, res = _rows(fx["test_mode"]["light"])
    d, r = E.hashimotoLightBatch(TEST_DATASET, d_cache, h, n, ctx)
    assert (d == mix).all() and (r == res).all()


@pytest.fixture(scope="module")
def series1000(small):
    """1,000 (hash, nonce) items and the model's hashimoto_full over its 32 KiB dataset (light == full)"""
    _, _, _, dataset = small
    h, n = _series(1000, 0xE7A5)
    d, r = M.hashimoto_full(TEST_DATASET, dataset, h, n)
    return h, n, d, r


@pytest.mark.parametrize("n", [0, 1, 2, 31, 32, 33, 63, 64, 65, 257, 1000])
def test_light_matches_full_at_wave_edges(ctx, small, series1000, n):
    """partial waves and odd pair counts of the two-lane mapping; rows = 16 in the cache, 256 mix rows"""
    from gsv import ethash as E
    _, d_cache, _, _ = small
    h, nn, want_d, want_r = series1000
    d, r = E.hashimotoLightBatch(TEST_DATASET, d_cache, h[:n], nn[:n], ctx)
    assert d.shape == (n, 32) and (d == want_d[:n]).all() and (r == want_r[:n]).all()


# ---------------------------------------------------------------- dataset items
def test_items_test_mode(ctx, fx, small):
    from gsv import ethash as E
    _, d_cache, _, dataset = small
    want = np.frombuffer(M.item_bytes(dataset), np.uint8).reshape(512, 64)
    got = E.generateDatasetItems(d_cache, 0, 512, ctx)
    assert (got == want).all()
    assert M.keccak256_bytes(got.tobytes()).hex() == fx["test_mode"]["dataset_digest"]
    for first, count in ((0, 1), (1, 63), (64, 448)):
        assert (E.generateDatasetItems(d_cache, first, count, ctx) == want[first:first + count]).all()
    assert E.generateDatasetItems(d_cache, 5, 0, ctx).shape == (0, 64)


def test_items_epoch0(ctx, fx, full):
    """the 7 fixture indices, each alone and inside a 256-item range around it where one exists"""
    from gsv import ethash as E
    d_cache, dataset_bytes = full[0]
    last = dataset_bytes // 64 - 1
    assert fx["items"][-1]["index"] == last
    for r in fx["items"]:
        want = bytes.fromhex(r["bytes"])
        assert E.generateDatasetItems(d_cache, r["index"], 1, ctx)[0].tobytes() == want, r["index"]
        first = max(0, min(r["index"] - 128, last + 1 - 256))
        got = E.generateDatasetItems(d_cache, first, 256, ctx)
        assert got[r["index"] - first].tobytes() == want, r["index"]


# ---------------------------------------------------------------- real row counts
def test_light_real_sizes_dev_form(ctx, fx, full):
    from gsv import ethash as E
    for block, count in ((0, 16), (30000, 8)):
        d_cache, dataset_bytes = full[block]
        h, n, mix, res = _rows(fx["light"][str(block)])
        assert len(n) == count
        d, r = E.hashimotoLightBatch(dataset_bytes, d_cache, h, n, ctx)
        assert (d == mix).all() and (r == res).all()


def test_light_real_sizes_host_form_by_block_number(ctx, fx):
    from gsv import ethash as E
    a, b = _rows(fx["light"]["0"]), _rows(fx["light"]["30000"])
    h = np.concatenate([a[0], b[0]])
    n = np.concatenate([a[1], b[1]])
    numbers = np.array([29999] * 16 + [30000 + k for k in range(8)], np.uint64)
    order = np.random.default_rng(5).permutation(24)
    d, r = E.Ethash(ctx=ctx).hashimotoLight(numbers[order], h[order], n[order])
    assert (d == np.concatenate([a[2], b[2]])[order]).all() and (r == np.concatenate([a[3], b[3]])[order]).all()
    assert ctx.ethash_caches() <= 3


def test_light_wide_indices(ctx):
    """a synthetic cache of 4,194,301 rows (256 MiB of random bytes) under a 2^38-byte dataset: where 32-bit
    index or byte-offset arithmetic would wrap"""
    from gsv import ethash as E
    rows = 4194301
    rng = np.random.default_rng(0x3838)
    raw = rng.integers(0, 2**32, rows * 16, dtype=np.uint32)
    d_cache = _dev(ctx, raw.view(np.uint8))
    h, n = _series(8, 0x77)
    want_d, want_r = M.hashimoto_light(1 << 38, raw.reshape(rows, 16), h, n)
    d, r = E.hashimotoLightBatch(1 << 38, d_cache, h, n, ctx)
    assert (d == want_d).all() and (r == want_r).all()


# ---------------------------------------------------------------- verify
def _be32(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "big") for v in values), np.uint8).reshape(-1, 32)


def test_verify_seal_statuses(ctx, small, series1000):
    import torch
    from gsv import _lib
    _, d_cache, _, _ = small
    h, nn, mix, res = (a[:64] for a in series1000)
    r = [int.from_bytes(x.tobytes(), "big") for x in res]
    assert all(v > 1 for v in r)
    d_h, d_n = _dev(ctx, h), _dev(ctx, nn)

    def run(mixes, diffs):
        st = torch.full((64,), GUARD, dtype=torch.uint8, device=d_h.device)
        d_mix, d_diff = _dev(ctx, mixes), _dev(ctx, _be32(diffs))
        ctx.ethash_verify_seal_batch_dev(d_cache, TEST_DATASET, d_h, d_n, d_mix, d_diff, st)
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
    # mixed in one batch
    diffs = [MAXU // v + (k % 2) for k, v in enumerate(r)]
    want = np.array([_lib.ST_INVALID_POW if k % 2 else _lib.ST_OK for k in range(64)], np.uint8)
    assert (run(mix, diffs) == want).all()


def test_verify_seal_python(ctx, series1000):
    from gsv import _lib
    from gsv import ethash as E
    eng = E.Ethash(test_mode=True, ctx=ctx)  # block 0 in test mode: the 1 KiB cache of a zero seed
    h, nn, mix, res = (a[:4] for a in series1000)
    r = [int.from_bytes(x.tobytes(), "big") for x in res]
    args = (0, h[0].tobytes(), int(nn[0]), mix[0].tobytes())
    eng.VerifySeal(*args, MAXU // r[0])
    eng.VerifySeal(*args, 1)
    with pytest.raises(E.ErrInvalidPoW):
        eng.VerifySeal(*args, MAXU // r[0] + 1)
    with pytest.raises(E.ErrInvalidPoW):
        eng.VerifySeal(*args, 1 << 256)
    with pytest.raises(E.ErrInvalidDifficulty):
        eng.VerifySeal(*args, 0)
    with pytest.raises(E.ErrInvalidDifficulty):
        eng.VerifySeal(0, h[0].tobytes(), int(nn[0]), bytes(32), -5)
    with pytest.raises(E.ErrInvalidMixDigest):
        eng.VerifySeal(0, h[0].tobytes(), int(nn[0]), mix[1].tobytes(), 1)
    st = eng.VerifySeals([0] * 4, h, nn, mix, [MAXU // r[0], 0, MAXU // r[2] + 1, 1 << 300])
    assert list(st) == [_lib.ST_OK, _lib.ST_INVALID_DIFFICULTY, _lib.ST_INVALID_POW, _lib.ST_INVALID_POW]


# ---------------------------------------------------------------- the host form across epochs
def test_host_form_across_epochs(ctx, series1000):
    from gsv import _lib
    from gsv import ethash as E
    h, nn = series1000[0][:40], series1000[1][:40]
    epochs = [0, 1, 2, 3, 7]
    numbers = np.array([epochs[k % 5] * 30000 + 17 * k for k in range(40)], np.uint64)
    eng = E.Ethash(test_mode=True, ctx=ctx)
    d, r = eng.hashimotoLight(numbers, h, nn)
    assert ctx.ethash_caches() == _lib.ETHASH_MAX_CACHES
    for e in epochs:
        pick = np.nonzero(numbers // 30000 == e)[0]
        cache = E.generateCache(1024, E.seedHash(e * 30000))
        wd, wr = E.hashimotoLightBatch(TEST_DATASET, cache, h[pick], nn[pick], ctx)
        assert (d[pick] == wd).all() and (r[pick] == wr).all(), e
    # the same through the verify form: every item's own digest, difficulty 1
    st = eng.VerifySeals(numbers, h, nn, d, [1] * 40)
    assert (st == _lib.ST_OK).all()
    assert ctx.ethash_caches() == _lib.ETHASH_MAX_CACHES


# ---------------------------------------------------------------- the _dev contract
def test_dev_form_contract(ctx, small, series1000):
    import torch
    from gsv import GsvError, _lib
    _, d_cache, _, _ = small
    dev = d_cache.device
    n = 65
    h, nn, want_d, want_r = (a[:n] for a in series1000)
    # inputs at byte offsets that are 4- and 8-aligned but not 16-aligned; outputs at odd offsets inside
    # guard bytes
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

    def check(wd, wr):
        m, r = mbuf.cpu().numpy(), rbuf.cpu().numpy()
        assert (m[17:17 + 32 * n].reshape(n, 32) == wd).all() and (r[3:3 + 32 * n].reshape(n, 32) == wr).all()
        assert (m[:17] == GUARD).all() and (m[17 + 32 * n:] == GUARD).all()
        assert (r[:3] == GUARD).all() and (r[3 + 32 * n:] == GUARD).all()

    ctx.set_timing(True)
    try:
        ctx.reset_timing()
        ctx.ethash_light_batch_dev(d_cache, TEST_DATASET, d_h, d_n, d_mix, d_res, stream=cs, n=n)
        cs.synchronize()
        ms, launches = ctx.kernel_time(_lib.K_ETHASH_LIGHT)
        assert launches == 1 and ms > 0
    finally:
        ctx.set_timing(False)
        ctx.reset_timing()
    check(want_d, want_r)

    # refused: a hash row off 4-byte alignment, nonces off 8-byte alignment, sizes outside the rules
    def refused(*a, **k):
        with pytest.raises(GsvError) as e:
            ctx.ethash_light_batch_dev(*a, **k)
        assert e.value.code == _lib.E_INVALID_ARG
    refused(d_cache, TEST_DATASET, hbuf[2:], d_n, d_mix, d_res, n=n)
    refused(d_cache, TEST_DATASET, d_h, nbuf[4:], d_mix, d_res, n=n)
    refused(d_cache[:1000], TEST_DATASET, d_h, d_n, d_mix, d_res, n=n)
    refused(d_cache[:0], TEST_DATASET, d_h, d_n, d_mix, d_res, n=n)
    refused(d_cache[4:4 + 64], TEST_DATASET, d_h, d_n, d_mix, d_res, n=n)  # a cache off 16-byte alignment
    for size in (0, 64, 128 + 64, (1 << 38) + 128):
        refused(d_cache, size, d_h, d_n, d_mix, d_res, n=n)
    with pytest.raises(GsvError):
        ctx.ethash_dataset_items_dev(d_cache, (1 << 32) - 1, 2, mbuf)
    ctx.ethash_light_batch_dev(d_cache, TEST_DATASET, None, None, None, None, n=0)  # n == 0: no launch
    torch.cuda.synchronize()
    check(want_d, want_r)

    # captured on an explicit stream (nothing allocated, nothing synchronised inside), replayed twice with
    # changed nonces
    g = torch.cuda.CUDAGraph()
    caches_before = ctx.ethash_caches()
    with torch.cuda.graph(g, stream=cs):
        ctx.ethash_light_batch_dev(d_cache, TEST_DATASET, d_h, d_n, d_mix, d_res, stream=cs, n=n)
    assert ctx.ethash_caches() == caches_before
    for shift in (1, 2):
        nn2 = np.roll(nn, shift)
        wd, wr = M.hashimoto_full(TEST_DATASET, small[3], h, nn2)
        d_n.copy_(_dev(ctx, nn2.view(np.uint8)))
        mbuf.fill_(GUARD)
        rbuf.fill_(GUARD)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check(wd, wr)
