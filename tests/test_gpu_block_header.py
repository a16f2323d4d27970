"""GPU tests of the block-header path (include/gsv.h, "block headers"): the header's RLP, Header.Hash() /
HashNoNonce(), CalcDifficulty and Ethash.VerifyHeaders.  Expected values come from the model
(tests/block_header_model.py, pinned by tests/test_block_header_cpu.py to the reference's two real headers and to
expectations written by hand), the fixture (tests/golden/block_headers.json) and the numpy ethash model, never
from the library.

The two real headers.  Their parents are in no file of the reference (a header's parent is whatever hashes to its
ParentHash, so none can be made up), so VerifyHeaders itself can only answer GSV_ST_UNKNOWN_ANCESTOR for them.
Their seals run through the new code all the same: the device chain decodes the RLP, makes HashNoNonce, the nonce,
the mix digest and the difficulty row on the device, and the seal kernel runs over exactly those arrays."""
import numpy as np
import pytest

import block_header_cases as C
import block_header_model as B
import ethash_model as M
from conftest import golden

pytestmark = pytest.mark.gpu

GUARD = 0xEE
TEST_DATASET = 32 * 1024
U256 = (1 << 256) - 1


@pytest.fixture(scope="module")
def fx():
    return golden("block_headers.json")


def lib_config(cfg: B.Config):
    from gsv import params as P
    return P.ChainConfig(HomesteadBlock=cfg.homestead, DAOForkBlock=cfg.dao, DAOForkSupport=cfg.dao_support,
                         EIP150Block=cfg.eip150, EIP150Hash=cfg.eip150_hash, ByzantiumBlock=cfg.byzantium)


def _rows(list_of_bytes):
    return np.frombuffer(b"".join(list_of_bytes), np.uint8).reshape(len(list_of_bytes), -1)


def _want_rows(wants):
    return _rows([B.want_row(w) for w in wants])


def _dev(ctx, a):
    import torch
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(torch.device("cuda", ctx.device))


def _model_rows(blobs):
    """what the device chain writes per header: HashNoNonce, nonce, mix digest, difficulty row, Number, Hash"""
    hnn, nonce, mix, diff, num, hsh = [], [], [], [], [], []
    for b in blobs:
        st, h = B.decode_status(b)
        ok = st == B.ST_OK
        hnn.append(B.hash_no_nonce(h) if h else bytes(32))
        hsh.append(B.header_hash(b) if h else bytes(32))
        nonce.append(B.nonce_number(h) if h else 0)
        mix.append(h["MixDigest"] if h else bytes(32))
        diff.append(h["Difficulty"].to_bytes(32, "big") if ok or (h and h["Difficulty"] <= U256) else bytes(32))
        num.append(h["Number"] if ok or (h and h["Number"] <= B.U64) else 0)
    return _rows(hnn), np.array(nonce, np.uint64), _rows(mix), _rows(diff), np.array(num, np.uint64), _rows(hsh)


class DevChain:
    """rules -> (seal) -> merge over torch tensors, every output in a guarded buffer at an odd offset"""

    def __init__(self, ctx, n, total, parent_len):
        import torch
        import gsv
        self.ctx, self.n = ctx, n
        dev = torch.device("cuda", ctx.device)
        z = lambda size, fill=0: torch.full((size,), fill, dtype=torch.uint8, device=dev)  # noqa: E731
        self.rlp = z(total + 8)
        self.off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        self.parent = z(parent_len) if parent_len else None
        self.work = z(gsv.block_header_work_bytes(n))
        self.hnn_buf, self.nonce_buf = z(4 + 32 * n + 16, GUARD), z(8 + 8 * n + 16, GUARD)
        self.hnn, self.nonce = self.hnn_buf[4:4 + 32 * n], self.nonce_buf[8:8 + 8 * n]
        self.num_buf = z(8 + 8 * n + 16, GUARD)
        self.number = self.num_buf[8:8 + 8 * n]
        self.bufs = {k: z(64 + w * n, GUARD) for k, w in (("mix", 32), ("diff", 32), ("hash", 32), ("want", 32),
                                                         ("pre", 1), ("post", 1), ("seal", 1), ("status", 1))}
        self.at = {"mix": 17, "diff": 3, "hash": 5, "want": 31, "pre": 1, "post": 7, "seal": 9, "status": 13}
        self.width = {"mix": 32, "diff": 32, "hash": 32, "want": 32, "pre": 1, "post": 1, "seal": 1, "status": 1}

    def view(self, k):
        return self.bufs[k][self.at[k]:self.at[k] + self.width[k] * self.n]

    def load(self, blobs, parent):
        flat = np.frombuffer(b"".join(blobs), np.uint8)
        off = np.zeros(len(blobs) + 1, np.uint64)
        np.cumsum([len(b) for b in blobs], out=off[1:])
        self.rlp[:flat.size].copy_(_dev(self.ctx, flat))
        self.off.copy_(_dev(self.ctx, off))
        if parent:
            self.parent.copy_(_dev(self.ctx, np.frombuffer(parent, np.uint8)))

    def rules(self, config, now, stream=None, **k):
        a = dict(rlp_t=self.rlp, off_t=self.off, n=self.n, parent_t=self.parent, now=now, work_t=self.work,
                 hnn_t=self.hnn, nonce_t=self.nonce, mix_t=self.view("mix"), difficulty_t=self.view("diff"),
                 pre_t=self.view("pre"), post_t=self.view("post"), hash_t=self.view("hash"), number_t=self.number,
                 expected_t=self.view("want"), stream=stream)
        a.update(k)
        self.ctx.block_header_rules_dev(config, **a)

    def seal(self, cache_t, dataset_bytes, stream=None):
        self.ctx.ethash_verify_seal_batch_dev(cache_t, dataset_bytes, self.hnn, self.nonce, self.view("mix"),
                                              self.view("diff"), self.view("seal"), stream=stream, n=self.n)

    def merge(self, seal=True, seals_t=None, stream=None):
        self.ctx.block_header_merge_dev(self.view("pre"), self.view("seal") if seal else None, seals_t, self.view("post"),
                                        self.view("status"), n=self.n, stream=stream)

    def get(self, k):
        """the rows of output k, after checking the guard bytes around them"""
        b = self.bufs[k].cpu().numpy()
        lo, hi = self.at[k], self.at[k] + self.width[k] * self.n
        assert (b[:lo] == GUARD).all() and (b[hi:] == GUARD).all(), k
        return b[lo:hi].reshape(self.n, -1) if self.width[k] > 1 else b[lo:hi]

    def get_seal_inputs(self):
        h, nn, nu = self.hnn_buf.cpu().numpy(), self.nonce_buf.cpu().numpy(), self.num_buf.cpu().numpy()
        n = self.n
        assert (h[:4] == GUARD).all() and (h[4 + 32 * n:] == GUARD).all()
        assert (nn[:8] == GUARD).all() and (nn[8 + 8 * n:] == GUARD).all()
        assert (nu[:8] == GUARD).all() and (nu[8 + 8 * n:] == GUARD).all()
        return (h[4:4 + 32 * n].reshape(n, 32), nn[8:8 + 8 * n].copy().view(np.uint64),
                nu[8:8 + 8 * n].copy().view(np.uint64))


def _chain_of(blobs, parent, ctx):
    import torch
    d = DevChain(ctx, len(blobs), sum(len(b) for b in blobs), len(parent or b""))
    d.load(blobs, parent)
    torch.cuda.synchronize()
    return d


# ---------------------------------------------------------------- 1. the two reference headers
def test_reference_headers_hashes(ctx, fx):
    from gsv import types as T
    blobs = [bytes.fromhex(r["rlp"]) for r in fx["reference"]]
    h, hnn, st = T.HeaderHashes(blobs, ctx)
    assert (st == 0).all()
    assert [x.tobytes().hex() for x in h] == [r["hash"] for r in fx["reference"]]
    assert h[0].tobytes().hex() == "0a5843ac1cb04865017cb35a57b50b07084e5fcee39b5acadade33149f4fff9e"  # block_test.go:49
    assert [x.tobytes().hex() for x in hnn] == [r["hash_no_nonce"] for r in fx["reference"]]


@pytest.mark.parametrize("which", [0, 1])
def test_reference_header_seal_through_the_device_chain(ctx, fx, which):
    """block 1 over the real epoch-0 cache, mainnet block 3,311,058 over one epoch-110 cache generation: decode ->
    seal -> merge, the seal's status the one the reference's libethash gave (the fixture's)"""
    import torch
    from gsv import _lib
    from gsv import ethash as E
    from gsv import params as P
    r = fx["reference"][which]
    blob = bytes.fromhex(r["rlp"])
    h = B.decode_header(blob)
    # a made-up parent: right Number, earlier Time; its hash cannot be the header's ParentHash
    parent = B.encode_header(B.new_header(Number=h["Number"] - 1, Time=h["Time"] - 14, Difficulty=h["Difficulty"],
                                          GasLimit=h["GasLimit"]))
    cfg = P.MainnetChainConfig
    d = _chain_of([blob], parent, ctx)
    cache = E._device_cache(E.generateCache(E.cacheSize(h["Number"]), E.seedHash(h["Number"])), ctx)
    d.rules(cfg, h["Time"])
    d.seal(cache, E.datasetSize(h["Number"]))
    d.merge()
    torch.cuda.synchronize()
    hnn, nonce, number = d.get_seal_inputs()
    assert hnn[0].tobytes().hex() == r["hash_no_nonce"] and nonce[0] == r["nonce"] and number[0] == r["number"]
    assert d.get("mix")[0].tobytes() == h["MixDigest"] and d.get("diff")[0].tobytes() == h["Difficulty"].to_bytes(32, "big")
    assert d.get("seal")[0] == r["seal_status"]
    assert d.get("pre")[0] == d.get("status")[0] == _lib.ST_UNKNOWN_ANCESTOR
    # the host form agrees: no ancestor, whatever the seal
    eng = E.Ethash(ctx=ctx)
    assert eng.VerifyHeaders(cfg, [blob], [True], parent, now=h["Time"])[0] == _lib.ST_UNKNOWN_ANCESTOR
    with pytest.raises(E.ErrUnknownAncestor):
        eng.VerifyHeader(cfg, blob, parent, now=h["Time"])
    if which == 0:
        # and the seal's host form over the hash the new call made (the context's own epoch-0 cache)
        _, hnn2, _ = ctx.block_header_hash_batch([blob])
        assert eng.VerifySeals([1], hnn2, [r["nonce"]], [h["MixDigest"]], [h["Difficulty"]])[0] == r["seal_status"]


# ---------------------------------------------------------------- 2. lengths
def test_hashes_at_every_length(ctx):
    hs = C.length_sweep()
    blobs = [B.encode_header(h) for h in hs]
    assert {543, 544, 545, 627, 628, 629} <= {len(b) for b in blobs}
    h, hnn, st = ctx.block_header_hash_batch(blobs)
    assert (st == 0).all()
    for k, (b, hd) in enumerate(zip(blobs, hs)):
        assert h[k].tobytes() == B.header_hash(b), (k, len(b))
        assert hnn[k].tobytes() == B.hash_no_nonce(hd), (k, len(b))
    # each header alone and at another byte offset in the batch: the loader realigns
    for k in (0, 33, len(blobs) - 5):
        h1, n1, s1 = ctx.block_header_hash_batch([b"\x80" * (k % 4 + 1), blobs[k]])
        assert s1.tolist() == [B.ST_BAD_RLP, 0] and not h1[0].any() and not n1[0].any()
        assert h1[1].tobytes() == B.header_hash(blobs[k]) and n1[1].tobytes() == B.hash_no_nonce(hs[k])


# ---------------------------------------------------------------- 3. the decode corpus
def test_decode_corpus(ctx):
    from gsv import params as P
    corpus = C.decode_corpus()
    blobs = [b for _, b, _ in corpus]
    h, hnn, st = ctx.block_header_hash_batch(blobs)
    for k, (name, blob, want) in enumerate(corpus):
        assert st[k] == want == B.decode_status(blob)[0], name
        if want == B.ST_BAD_RLP:
            assert not h[k].any() and not hnn[k].any(), name
        else:
            assert h[k].tobytes() == B.header_hash(blob), name
            assert hnn[k].tobytes() == B.hash_no_nonce(B.decode_header(blob)), name
    # as a segment: the decode status where there is one, no ancestor for the rest (nothing links)
    got = ctx.ethash_verify_headers_batch(P.TestChainConfig, blobs, [False] * len(blobs), blobs[0], now=1 << 40)
    want, _ = B.verify_headers(C.TEST_CONFIG, blobs, blobs[0], 1 << 40)
    assert got.tolist() == want
    assert set(want) == {B.ST_BAD_RLP, B.ST_HEADER_TOO_WIDE, B.ST_UNKNOWN_ANCESTOR}


# ---------------------------------------------------------------- 4. batch shapes
@pytest.fixture(scope="module")
def long_chain():
    """a parent and 300 valid headers under TEST_CONFIG with their model verdicts"""
    parent = B.new_header(Difficulty=1 << 24, Number=41, GasLimit=6000000, Time=1500000000, Extra=b"long")
    pb = B.encode_header(parent)
    blobs, prev, prev_blob = [], parent, pb
    for k in range(300):
        h = C.child(C.TEST_CONFIG, prev, prev_blob, dt=1 + (7 * k) % 23, salt=k, Extra=bytes(range(k % 33)),
                    GasLimit=prev["GasLimit"] + (k % 5) - 2, UncleHash=B.EMPTY_UNCLE_HASH if k % 2 else bytes([k & 255]) * 32)
        blobs.append(B.encode_header(h))
        prev, prev_blob = h, blobs[-1]
    now = prev["Time"]
    st, wants = B.verify_headers(C.TEST_CONFIG, blobs, pb, now)
    assert st == [0] * 300
    return pb, blobs, now, wants


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257])
def test_batch_shapes(ctx, long_chain, n):
    """the parent link crosses wave and workgroup edges; from the segment's start and from inside the chain"""
    from gsv import params as P
    pb, blobs, now, wants = long_chain
    for first in (0, 300 - n):
        seg = blobs[first:first + n]
        parent = blobs[first - 1] if first else pb
        st, h, want = ctx.ethash_verify_headers_batch(P.TestChainConfig, seg, [False] * n, parent, now, want_hash=True,
                                                      want_expected=True)
        assert (st == 0).all(), (n, first, st.tolist())
        assert (h == _rows([B.header_hash(b) for b in seg])).all()
        assert (want == _want_rows(wants[first:first + n])).all()
    # a link broken in the middle: that header alone has no ancestor, and it still parents the one behind it
    if n >= 3:
        k = n // 2
        broken = B.decode_header(blobs[k])
        broken["ParentHash"] = bytes(x ^ 0x80 for x in broken["ParentHash"])
        bb = B.encode_header(broken)
        behind = B.encode_header(C.child(C.TEST_CONFIG, broken, bb, salt=5))
        seg = blobs[:k] + [bb, behind] + blobs[k + 2:n]
        st = ctx.ethash_verify_headers_batch(P.TestChainConfig, seg, [False] * n, pb, now + 10)
        want, _ = B.verify_headers(C.TEST_CONFIG, seg, pb, now + 10)
        assert st.tolist() == want and want[k] == B.ST_UNKNOWN_ANCESTOR and want[k + 1] == B.ST_OK
        assert k + 2 >= n or want[k + 2] == B.ST_UNKNOWN_ANCESTOR


@pytest.mark.parametrize("key", ["chain40", "forks", "forks_no_dao"])
def test_generated_chains_pass(ctx, fx, key):
    from gsv import ethash as E
    ch = fx[key]
    cfg = C.config_of(ch["config"])
    blobs = [bytes.fromhex(x) for x in ch["headers"]]
    parent = bytes.fromhex(ch["parent"])
    seals = [k in ch["sealed"] for k in range(len(blobs))]
    eng = E.Ethash(test_mode=True, ctx=ctx)
    st = eng.VerifyHeaders(lib_config(cfg), blobs, seals, parent, now=ch["now"])
    assert (st == 0).all(), st.tolist()
    st, h, want = ctx.ethash_verify_headers_batch(lib_config(cfg), blobs, seals, parent, ch["now"], True, True, True)
    assert (st == 0).all() and [x.tobytes().hex() for x in h] == ch["hash"]
    assert [int.from_bytes(x.tobytes(), "big") for x in want] == ch["difficulty"]
    assert eng.VerifyHeaders(lib_config(cfg), blobs, seals, None, now=ch["now"]).tolist() == \
        [B.ST_UNKNOWN_ANCESTOR] + [0] * (len(blobs) - 1)
    eng.VerifyHeader(lib_config(cfg), blobs[0], parent, seal=seals[0], now=ch["now"])


def test_dao_and_fork_hash_verdicts(ctx, fx):
    a, b = fx["forks"], fx["forks_no_dao"]
    parent = bytes.fromhex(a["parent"])
    for chain in (a, b):
        blobs = [bytes.fromhex(x) for x in chain["headers"]]
        for cfg_of in (a, b):
            for drop_dao, zero_hash in ((False, False), (True, False), (True, True)):
                cfg = C.config_of(cfg_of["config"])
                if drop_dao:
                    cfg.dao = None
                if zero_hash:
                    cfg.eip150_hash = bytes(32)
                want, _ = B.verify_headers(cfg, blobs, parent, a["now"])
                got = ctx.ethash_verify_headers_batch(lib_config(cfg), blobs, [False] * 16, parent, a["now"])
                assert got.tolist() == want
    seen = set()
    for chain, cfg_of in ((a, b), (b, a)):
        cfg = C.config_of(cfg_of["config"])
        seen |= set(B.verify_headers(cfg, [bytes.fromhex(x) for x in chain["headers"]], parent, a["now"])[0])
    assert {B.ST_BAD_PRO_DAO_EXTRA, B.ST_BAD_NO_DAO_EXTRA} <= seen


# ---------------------------------------------------------------- 5. one failure per check
@pytest.fixture(scope="module")
def anchor():
    parent = B.new_header(Difficulty=1 << 20, Number=7, GasLimit=5000000, Time=1500000000, Extra=b"anchor")
    return parent, B.encode_header(parent), 1500000000 + 100000


def test_each_check_fails_alone_and_pairs_show_the_order(ctx, anchor):
    from gsv import _lib
    from gsv import ethash as E
    from gsv import params as P
    parent, pb, now = anchor
    eng = E.Ethash(test_mode=True, ctx=ctx)
    for k, (name, over, want) in enumerate(C.rule_cases(parent, now)):
        blobs, at = C.rule_segment(parent, pb, over, 3 * k)
        model, wants = B.verify_headers(C.TEST_CONFIG, blobs, pb, now)
        st, _, exp = ctx.ethash_verify_headers_batch(P.TestChainConfig, blobs, [False] * 3, pb, now, True, False, True)
        assert st.tolist() == model and st[at] == want, (name, st.tolist(), model)
        assert (exp == _want_rows(wants)).all(), name  # an invalid header still parents its child
        # a bad seal behind an earlier failure reports the earlier rule; asked for on a valid header, the seal
        if want != B.ST_OK:
            assert eng.VerifyHeaders(P.TestChainConfig, blobs, [False, True, False], pb, now)[at] == want, name
        else:
            assert eng.VerifyHeaders(P.TestChainConfig, blobs, [False, True, False], pb, now)[at] == \
                _lib.ST_INVALID_MIX_DIGEST, name
    errs = {B.ST_EXTRA_TOO_LONG: E.ErrExtraTooLong, B.ST_FUTURE_BLOCK: E.ErrFutureBlock,
            B.ST_ZERO_BLOCK_TIME: E.ErrZeroBlockTime, B.ST_WRONG_DIFFICULTY: E.ErrWrongDifficulty,
            B.ST_GAS_LIMIT_CAP: E.ErrGasLimitCap, B.ST_GAS_USED: E.ErrGasUsed,
            B.ST_GAS_LIMIT_BOUNDS: E.ErrGasLimitBounds, B.ST_INVALID_NUMBER: E.ErrInvalidNumber}
    done = set()
    for k, (name, over, want) in enumerate(C.rule_cases(parent, now)):
        if want in errs and want not in done:
            done.add(want)
            blobs, at = C.rule_segment(parent, pb, over, 3 * k)
            # alone, a wrong Number finds no parent: chain.GetHeader(ParentHash, Number - 1) (consensus.go:155)
            with pytest.raises(E.ErrUnknownAncestor if want == B.ST_INVALID_NUMBER else errs[want]):
                eng.VerifyHeader(P.TestChainConfig, blobs[at], blobs[at - 1], seal=False, now=now)
    assert done == set(errs)


def test_seals(ctx, fx):
    """test mode, epoch 0: seals false on a bad seal passes, seals true gives 17 / 18"""
    from gsv import _lib
    from gsv import ethash as E
    from gsv import params as P
    ch = fx["chain40"]
    blobs = [bytes.fromhex(x) for x in ch["headers"]]
    parent = bytes.fromhex(ch["parent"])
    # a header with the right mix digest for its nonce and, at difficulty >= 2^17, no proof of work
    efx = golden("ethash.json")
    cache = np.frombuffer(bytes.fromhex(efx["test_mode"]["cache0"]), np.uint8)
    dataset = M.dataset_item(M.words(cache), np.arange(512, dtype=np.uint32))
    last = B.decode_header(blobs[-1])
    x = C.child(C.TEST_CONFIG, last, blobs[-1], salt=77)
    mix, res = M.hashimoto_full(TEST_DATASET, dataset, np.frombuffer(B.hash_no_nonce(x), np.uint8).reshape(1, 32),
                                np.array([B.nonce_number(x)], np.uint64))
    x["MixDigest"] = mix[0].tobytes()
    assert int.from_bytes(res[0].tobytes(), "big") > U256 // x["Difficulty"]
    blobs = blobs + [B.encode_header(x)]
    n = len(blobs)
    # the seal's verdict per header from the numpy model
    hnn, nonce, mixes, diffs, _, _ = _model_rows(blobs)
    d, r = M.hashimoto_full(TEST_DATASET, dataset, hnn, nonce)
    seal = []
    for k in range(n):
        target = U256 // int.from_bytes(diffs[k].tobytes(), "big")
        seal.append(B.ST_INVALID_MIX_DIGEST if (d[k] != mixes[k]).any() else
                    B.ST_INVALID_POW if int.from_bytes(r[k].tobytes(), "big") > target else B.ST_OK)
    assert [k for k in range(n) if seal[k] == 0] == ch["sealed"] and seal[-1] == B.ST_INVALID_POW
    eng = E.Ethash(test_mode=True, ctx=ctx)
    now = ch["now"]
    for seals in (None, [True] * n, [False] * n, [k % 2 == 0 for k in range(n)], [k in ch["sealed"] for k in range(n)]):
        want, _ = B.verify_headers(C.TEST_CONFIG, blobs, parent, now, seal_status=seal, seals=seals)
        got = eng.VerifyHeaders(P.TestChainConfig, blobs, seals, parent, now)
        assert got.tolist() == want, seals
    assert set(B.verify_headers(C.TEST_CONFIG, blobs, parent, now, seal_status=seal)[0]) == \
        {0, _lib.ST_INVALID_MIX_DIGEST, _lib.ST_INVALID_POW}
    with pytest.raises(E.ErrInvalidPoW):
        eng.VerifyHeader(P.TestChainConfig, blobs[-1], blobs[-2], now=now)
    with pytest.raises(E.ErrInvalidMixDigest):
        eng.VerifyHeader(P.TestChainConfig, blobs[1], blobs[0], now=now)


# ---------------------------------------------------------------- 6. CalcDifficulty
def test_calc_difficulty(ctx):
    from gsv import _lib
    from gsv import ethash as E
    cases = C.difficulty_cases()
    groups = {}
    for cfg, time, parent in cases:
        groups.setdefault(id(cfg), (cfg, [], []))
        groups[id(cfg)][1].append(time)
        groups[id(cfg)][2].append(parent)
    over = 0
    for cfg, times, parents in groups.values():
        rows, st = ctx.calc_difficulty_batch(lib_config(cfg), times, [B.encode_header(p) for p in parents])
        for k, (t, p) in enumerate(zip(times, parents)):
            want = B.calc_difficulty(cfg, t, p)
            assert rows[k].tobytes() == B.want_row(want), (k, t, p["Number"], p["Difficulty"], p["Time"], want)
            assert st[k] == (_lib.ST_WRONG_DIFFICULTY if want > U256 else 0)
            over += want > U256
    assert over >= 8
    cfg, t, p = cases[5]
    assert E.CalcDifficulty(lib_config(cfg), t, B.encode_header(p), ctx) == B.calc_difficulty(cfg, t, p)
    with pytest.raises(OverflowError):
        E.CalcDifficulty(lib_config(B.Config()), 5, B.encode_header(B.new_header(Difficulty=131072, Number=B.U64)), ctx)
    with pytest.raises(E.ErrBadHeaderRLP):
        E.CalcDifficulty(lib_config(B.Config()), 5, b"\xc0", ctx)
    rows, st = ctx.calc_difficulty_batch(lib_config(cfg), [1, 2], [C.decode_corpus()[-3][1], b"\xc0"])
    assert st.tolist() == [B.ST_HEADER_TOO_WIDE, B.ST_BAD_RLP] and not rows.any()


# ---------------------------------------------------------------- 7. gas
def test_gas_limits(ctx):
    from gsv import params as P
    now = 1500000000 + 100000
    for pg, gl, gu, want in C.gas_cases():
        parent = B.new_header(Difficulty=1 << 20, Number=7, GasLimit=pg, Time=1500000000)
        pb = B.encode_header(parent)
        h = B.encode_header(C.child(C.TEST_CONFIG, parent, pb, GasLimit=gl, GasUsed=gu))
        assert B.verify_headers(C.TEST_CONFIG, [h], pb, now)[0] == [want]
        assert ctx.ethash_verify_headers_batch(P.TestChainConfig, [h], [False], pb, now).tolist() == [want], (pg, gl, gu)


# ---------------------------------------------------------------- 8. arguments
def test_host_forms_check_their_arguments(ctx, fx):
    from gsv import GsvError, _lib
    from gsv import params as P
    ch = fx["chain40"]
    blobs = [bytes.fromhex(x) for x in ch["headers"]][:3]
    parent = bytes.fromhex(ch["parent"])
    with pytest.raises(GsvError) as e:
        ctx.ethash_verify_headers_batch(P.TestChainConfig, blobs, None, parent, now=(1 << 63) + 1)
    assert e.value.code == _lib.E_INVALID_ARG
    assert ctx.ethash_verify_headers_batch(P.TestChainConfig, blobs, [False] * 3, parent, now=1 << 63).tolist() == [0] * 3
    assert ctx.ethash_verify_headers_batch(P.TestChainConfig, [], None, parent, now=5).shape == (0,)
    h, hnn, st = ctx.block_header_hash_batch([])
    assert h.shape == (0, 32) and st.shape == (0,)
    assert ctx.calc_difficulty_batch(P.TestChainConfig, [], [])[1].shape == (0,)


# ---------------------------------------------------------------- 9. the _dev contract
def test_dev_form_contract(ctx, fx):
    """guard bytes around every output at an odd offset, one launch per kernel id, the refusals, n == 0, and
    rules -> seal -> merge captured into a graph and replayed twice over changed input"""
    import torch
    from gsv import GsvError, _lib
    from gsv import params as P
    ch = fx["chain40"]
    base = [bytes.fromhex(x) for x in ch["headers"]]
    parent = bytes.fromhex(ch["parent"])
    now = ch["now"]
    cfg = P.TestChainConfig
    efx = golden("ethash.json")
    raw = np.frombuffer(bytes.fromhex(efx["test_mode"]["cache0"]), np.uint8)
    dataset = M.dataset_item(M.words(raw), np.arange(512, dtype=np.uint32))
    cache = _dev(ctx, raw)
    n = len(base)
    # room for the variants below: a corrupted header keeps its length
    d = _chain_of(base, parent, ctx)
    seals = np.array([k in ch["sealed"] or k % 7 == 0 for k in range(n)], np.uint8)
    d_seals = _dev(ctx, seals)
    cs = torch.cuda.Stream()

    def expect(blobs):
        hnn, nonce, mixes, diffs, num, hsh = _model_rows(blobs)
        dg, r = M.hashimoto_full(TEST_DATASET, dataset, hnn, nonce)
        seal = []
        for k in range(n):
            dv = int.from_bytes(diffs[k].tobytes(), "big")
            seal.append(B.ST_INVALID_DIFFICULTY if dv == 0 else B.ST_INVALID_MIX_DIGEST if (dg[k] != mixes[k]).any() else
                        B.ST_INVALID_POW if int.from_bytes(r[k].tobytes(), "big") > U256 // dv else B.ST_OK)
        st, wants, pre, post = B.verify_headers(C.TEST_CONFIG, blobs, parent, now, seal_status=seal,
                                                seals=seals.tolist(), detail=True)
        return dict(hnn=hnn, nonce=nonce, mix=mixes, diff=diffs, num=num, hash=hsh, seal=seal, status=st, want=wants,
                    pre=pre, post=post)

    def check(blobs):
        e = expect(blobs)
        hnn, nonce, number = d.get_seal_inputs()
        assert (hnn == e["hnn"]).all() and (nonce == e["nonce"]).all() and (number == e["num"]).all()
        assert (d.get("mix") == e["mix"]).all() and (d.get("diff") == e["diff"]).all()
        assert (d.get("hash") == e["hash"]).all() and (d.get("want") == _want_rows(e["want"])).all()
        assert d.get("pre").tolist() == e["pre"] and d.get("post").tolist() == e["post"]
        assert d.get("seal").tolist() == e["seal"] and d.get("status").tolist() == e["status"]
        return e

    def run(stream):
        d.rules(cfg, now, stream=stream)
        d.seal(cache, TEST_DATASET, stream=stream)
        d.merge(seals_t=d_seals, stream=stream)

    ctx.set_timing(True)
    try:
        ctx.reset_timing()
        run(cs)
        cs.synchronize()
        for kid in (_lib.K_BLOCK_HEADER, _lib.K_BLOCK_RULES, _lib.K_BLOCK_MERGE, _lib.K_ETHASH_LIGHT):
            ms, launches = ctx.kernel_time(kid)
            assert launches == 1 and ms > 0, kid
        # n == 0 enqueues nothing
        ctx.block_header_rules_dev(cfg, None, None, 0, None, now, None, None, None, None, None, None, None, stream=cs)
        ctx.block_header_merge_dev(None, None, None, None, None, n=0, stream=cs)
        cs.synchronize()
        for kid in (_lib.K_BLOCK_HEADER, _lib.K_BLOCK_RULES, _lib.K_BLOCK_MERGE):
            assert ctx.kernel_time(kid)[1] == 1, kid
    finally:
        ctx.set_timing(False)
        ctx.reset_timing()
    e = check(base)
    assert e["status"].count(0) >= len(ch["sealed"]) and B.ST_INVALID_MIX_DIGEST in e["status"]

    def refused(**k):
        with pytest.raises(GsvError) as err:
            d.rules(cfg, k.pop("now", now), **k)
        assert err.value.code == _lib.E_INVALID_ARG

    refused(hnn_t=d.hnn_buf[2:])        # hash rows off 4-byte alignment
    refused(nonce_t=d.nonce_buf[4:])    # nonces off 8-byte alignment
    refused(number_t=d.num_buf[4:])
    refused(work_t=d.work[8:])          # the work area off 16-byte alignment
    refused(off_t=d.off.view(torch.uint8)[4:])
    refused(now=(1 << 63) + 1)
    refused(rlp_t=None)
    refused(pre_t=None)
    with pytest.raises(GsvError):
        ctx.block_header_merge_dev(None, None, None, d.view("post"), d.view("status"), n=n)
    torch.cuda.synchronize()
    check(base)  # nothing was written by the refused calls

    # the optional outputs may be absent, and the merge without a seal array skips the seal
    for k in ("hash", "want"):
        d.bufs[k].fill_(GUARD)
    torch.cuda.synchronize()
    d.rules(cfg, now, stream=cs, hash_t=None, number_t=None, expected_t=None)
    d.merge(seal=False, stream=cs)
    cs.synchronize()
    assert (d.bufs["hash"].cpu().numpy() == GUARD).all() and (d.bufs["want"].cpu().numpy() == GUARD).all()
    assert d.get("status").tolist() == B.verify_headers(C.TEST_CONFIG, base, parent, now)[0]

    # captured on an explicit stream, replayed twice over changed headers of the same lengths
    before = (ctx.ethash_caches(), ctx.prepared_shapes())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        run(cs)
    assert (ctx.ethash_caches(), ctx.prepared_shapes()) == before
    for variant in (1, 2):
        blobs = list(base)
        k = 5 * variant
        h = B.decode_header(blobs[k])
        h["GasUsed"] = h["GasLimit"] + 1 if variant == 1 else h["GasUsed"]
        h["Coinbase"] = bytes([variant]) * 20  # another hash: the header behind it loses its ancestor
        enc = B.encode_header(h)
        if len(enc) != len(blobs[k]):
            h["GasUsed"] = B.decode_header(blobs[k])["GasUsed"]
            enc = B.encode_header(h)
        assert len(enc) == len(blobs[k])
        blobs[k] = enc
        blobs[20 + variant] = blobs[20 + variant][:-1] + b"\x00" if variant == 2 else blobs[20 + variant]
        d.load(blobs, parent)
        for buf in d.bufs.values():
            buf.fill_(GUARD)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        e = check(blobs)
        assert e["status"][k + 1] == B.ST_UNKNOWN_ANCESTOR
