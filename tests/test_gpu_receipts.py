"""GPU tests of the receipt path (include/gsv.h, "logs bloom and receipts"): bloom9, CreateBloom, the strict
receipt decode and the receipt half of ValidateState.  Expected values come from the model (tests/receipt_model.py,
pinned to the reference by tests/test_receipt_cpu.py), the shared cases (tests/receipt_cases.py) and the fixture
(tests/golden/receipts.json), never from the library."""
import random

import numpy as np
import pytest

import receipt_cases as C
import receipt_model as R
import tx_rules_model as RLP
from conftest import golden

pytestmark = pytest.mark.gpu

GUARD = 0xEE


def _rows(list_of_bytes, width):
    return np.frombuffer(b"".join(list_of_bytes), np.uint8).reshape(len(list_of_bytes), width)


def expect(lists, want=None):
    """the model's (status, blooms, roots, gas, receipt statuses) of a batch; want: per list (bloom, root, gas)"""
    st, bloom, root, gas, rst = [], [], [], [], []
    for k, lst in enumerate(lists):
        w = want[k] if want else (None, None, None)
        s, b, r, g, rs = R.validate(lst, *w)
        st.append(s), bloom.append(b), root.append(r), gas.append(g), rst.extend(rs)
    return st, _rows(bloom, 256), _rows(root, 32), gas, rst


def check_host(ctx, lists, want=None):
    e = expect(lists, want)
    cols = list(zip(*want)) if want else (None, None, None)
    st, rst, bloom, root, gas = ctx.receipts_verify_batch(lists, *cols)
    assert rst.tolist() == e[4]
    assert st.tolist() == e[0]
    assert (bloom == e[1]).all() and (root == e[2]).all() and gas.tolist() == e[3]
    return e


# ---------------------------------------------------------------- 1. bloom9
def test_bloom9_words_and_lengths(ctx):
    from gsv import types as T
    fx = golden("receipts.json")
    words = [bytes.fromhex(w["data"]) for w in fx["bloom9"]]
    got = T.Bloom9(words, ctx)
    assert got.dtype == np.uint16 and got.tolist() == [w["indexes"] for w in fx["bloom9"]]
    assert got[0].tolist() == [1303, 70, 1533] and got[7].tolist() == [896, 1975, 1665]  # bloom9_test.go's testtest
    rng = random.Random(3)
    msgs = [bytes(rng.getrandbits(8) for _ in range(n)) for n in list(range(0, 70)) + [135, 136, 137, 271, 272, 273, 1000]]
    assert T.Bloom9(msgs, ctx).tolist() == [R.bloom_indexes(m) for m in msgs]
    assert T.Bloom9([], ctx).shape == (0, 3)
    # TestBloom (bloom9_test.go:24-51) through BloomLookup
    acc = 0
    for w in (b"testtest", b"test", b"hallo", b"other"):
        acc |= R.bloom9(w)
    bloom = R.to_bloom(acc)
    assert T.BloomLookupBatch([bloom] * 6, [b"testtest", b"test", b"hallo", b"other", b"tes", b"lo"], ctx).tolist() == \
        [True, True, True, True, False, False]
    assert T.BloomLookup(bloom, b"hallo", ctx) and not T.BloomLookup(bloom, b"lo", ctx)


def test_bloom9_dev_form(ctx):
    """device offsets, data at an odd address, guard bytes around the rows, one launch, n == 0"""
    import torch
    from gsv import _lib
    dev = torch.device("cuda", ctx.device)
    rng = random.Random(4)
    msgs = [bytes(rng.getrandbits(8) for _ in range(rng.choice((0, 20, 32, 136, 200)))) for _ in range(300)]
    flat = np.frombuffer(b"".join(msgs), np.uint8)
    off = np.zeros(len(msgs) + 1, np.int64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    buf = torch.zeros(flat.size + 16, dtype=torch.uint8, device=dev)
    data = buf[5:5 + flat.size]
    data.copy_(torch.from_numpy(flat.copy()))
    assert data.data_ptr() % 2 == 1
    out = torch.full((8 + 6 * len(msgs) + 8,), GUARD, dtype=torch.uint8, device=dev)
    (stream,) = ctx.pipeline_streams(1)
    ctx.set_timing(True)
    try:
        ctx.reset_timing()
        ctx.bloom9_batch_dev(data, torch.from_numpy(off).to(dev), out[8:8 + 6 * len(msgs)], stream=stream)
        ctx.bloom9_batch_dev(None, None, None, n=0, stream=stream)
        stream.synchronize()
        assert ctx.kernel_time(_lib.K_BLOOM9)[1] == 1
    finally:
        ctx.set_timing(False)
        ctx.reset_timing()
        ctx.destroy_streams([stream])
    o = out.cpu().numpy()
    assert (o[:8] == GUARD).all() and (o[-8:] == GUARD).all()
    assert o[8:-8].copy().view(np.uint16).reshape(-1, 3).tolist() == [R.bloom_indexes(m) for m in msgs]


# ---------------------------------------------------------------- 2. decode
def test_decode_corpus(ctx):
    """every shape that decodes (0, 4 and 7 topics; data of 0 .. 65,536 bytes; the logs-list boundaries; the three
    status forms; the gas values) and one case per refusal, each as a list of its own"""
    from gsv import types as T
    corpus = C.decode_corpus()
    lists = [[b] for _, b, _ in corpus]
    e = check_host(ctx, lists)
    for k, (name, _, want) in enumerate(corpus):
        assert e[0][k] == want == e[4][k], name
    assert {n for n, _, _ in corpus} >= {"data 65536", "7 topics", "logs payload 56", "status 33 bytes", "gas 9 bytes",
                                         "bytes behind the list", "empty item"}
    # all of them in ONE list: the first failure decides, zero rows
    blobs = [b for _, b, _ in corpus]
    first_bad = next(s for _, _, s in corpus if s != R.ST_OK)
    st, rst, bloom, root, gas = ctx.receipts_verify_batch([blobs])
    assert st.tolist() == [first_bad] and rst.tolist() == [s for _, _, s in corpus]
    assert not bloom.any() and not root.any() and gas.tolist() == [0]
    # LogsBloom: a row per receipt
    rows, st = T.LogsBloom(blobs, ctx)
    for k, (name, b, want) in enumerate(corpus):
        assert st[k] == want, name
        assert rows[k].tobytes() == (R.logs_bloom(R.decode_receipt(b)["logs"]) if want == R.ST_OK else bytes(256)), name
    with pytest.raises(T.ErrBadReceipt):
        T.CreateBloom(blobs, ctx)


def test_fixture(ctx):
    fx = golden("receipts.json")
    lists = [[bytes.fromhex(x) for x in e["receipts"]] for e in fx["lists"]]
    st, rst, bloom, root, gas = ctx.receipts_verify_batch(lists)
    assert st.tolist() == [e["status"] for e in fx["lists"]]
    assert [b.tobytes().hex() for b in bloom] == [e["bloom"] for e in fx["lists"]]
    assert [r.tobytes().hex() for r in root] == [e["root"] for e in fx["lists"]]
    assert gas.tolist() == [e["gas_used"] for e in fx["lists"]]
    assert rst.tolist() == [s for e in fx["lists"] for s in e["receipt_status"]]
    assert root[0].tobytes() == R.EMPTY_ROOT and not bloom[0].any()  # the empty list


# ---------------------------------------------------------------- 3. list and launch shapes
@pytest.fixture(scope="module")
def shaped():
    """lists of 0, 1, 63, 64, 65 and 257 receipts: a few thousand bloom items"""
    lists = C.random_lists(11, [0, 1, 63, 64, 65, 257, 0, 2], max_logs=4)
    assert sum(C.count_items(lst) for lst in lists) > 3000
    return lists, expect(lists)


def test_list_shapes_bit_for_bit(ctx, shaped):
    from gsv import core
    lists, e = shaped
    st, rst, bloom, root, gas = ctx.receipts_verify_batch(lists)
    assert not st.any() and not rst.any()
    assert (bloom == e[1]).all() and (root == e[2]).all() and gas.tolist() == e[3]
    # each list alone, and the public call with the headers' values
    for k in (0, 2, 5):
        check_host(ctx, [lists[k]])
    st, b2, r2, g2 = core.ValidateReceipts(lists, bloom, root, gas, ctx)
    assert not st.any() and (b2 == bloom).all() and (r2 == root).all() and (g2 == gas).all()


def test_one_receipt_holds_every_log(ctx):
    """a receipt of 300 logs beside lists of receipts without logs: its items spread over lanes like any others"""
    rng = random.Random(21)
    logs = [(bytes(rng.getrandbits(8) for _ in range(20)), [bytes(rng.getrandbits(8) for _ in range(32))
                                                             for _ in range(k % 5)], bytes(k % 7)) for k in range(300)]
    full = R.encode_receipt(R.new_receipt(gas=5000000, logs=logs))
    empty = [R.encode_receipt(R.new_receipt(gas=21000 * (k + 1))) for k in range(70)]
    lists = [empty[:3], empty[:1] + [full] + empty[1:2], empty, [full], []]
    check_host(ctx, lists)


def test_one_address_a_thousand_times(ctx):
    """every atomic hits the same three dwords; the bloom is that of a single copy"""
    one = (C.addr(40), [], b"")
    many = R.encode_receipt(R.new_receipt(gas=1, logs=[one] * 1000))
    spread = [R.encode_receipt(R.new_receipt(gas=k + 1, logs=[one] * 4)) for k in range(250)]
    single = R.logs_bloom([one])
    assert sum(bin(x).count("1") for x in single) == 3
    st, _, bloom, _, _ = ctx.receipts_verify_batch([[many], spread, [many] + spread])
    assert not st.any()
    for row in bloom:
        assert row.tobytes() == single


# ---------------------------------------------------------------- 4. the compare
def test_each_compare_status_and_their_order(ctx, shaped):
    from gsv import core
    lists, e = shaped
    lists = lists[:5]
    good = [(e[1][k].tobytes(), e[2][k].tobytes(), e[3][k]) for k in range(5)]
    flip = lambda b: bytes([b[0] ^ 0x80]) + b[1:]  # noqa: E731
    cases = {
        "all right": (lambda b, r, g: (b, r, g), R.ST_OK),
        "gas": (lambda b, r, g: (b, r, g + 1), R.ST_GAS_USED_MISMATCH),
        "bloom": (lambda b, r, g: (flip(b), r, g), R.ST_INVALID_BLOOM),
        "bloom, last byte": (lambda b, r, g: (b[:-1] + bytes([b[-1] ^ 1]), r, g), R.ST_INVALID_BLOOM),
        "root": (lambda b, r, g: (b, flip(r), g), R.ST_INVALID_RECEIPT_ROOT),
        "root, last byte": (lambda b, r, g: (b, r[:-1] + bytes([r[-1] ^ 1]), g), R.ST_INVALID_RECEIPT_ROOT),
        "gas before bloom": (lambda b, r, g: (flip(b), r, g + 1), R.ST_GAS_USED_MISMATCH),
        "gas before root": (lambda b, r, g: (b, flip(r), g + 1), R.ST_GAS_USED_MISMATCH),
        "bloom before root": (lambda b, r, g: (flip(b), flip(r), g), R.ST_INVALID_BLOOM),
    }
    for name, (f, want) in cases.items():
        # list k gets the altered values, the others the right ones
        for k in (1, 4):
            w = [f(*good[j]) if j == k else good[j] for j in range(5)]
            ex = check_host(ctx, lists, w)
            assert ex[0] == [want if j == k else 0 for j in range(5)], name
    # each want_* absent alone, and all three: the compare is skipped
    wrong = [(flip(b), flip(r), g + 1) for b, r, g in good]
    for drop, want in (((2,), R.ST_INVALID_BLOOM), ((0, 2), R.ST_INVALID_RECEIPT_ROOT), ((0, 1, 2), R.ST_OK),
                       ((1,), R.ST_GAS_USED_MISMATCH)):
        cols = [None if j in drop else col for j, col in enumerate(zip(*wrong))]
        st, bloom, root, gas = core.ValidateReceipts(lists, *cols, ctx=ctx)
        assert st.tolist() == [want] * 5, drop
        assert (bloom == e[1][:5]).all() and (root == e[2][:5]).all() and gas.tolist() == e[3][:5]
    # a failed receipt comes before every compare
    bad = [lists[2][:5] + [C.raw(status=b"\x02")] + lists[2][5:]]
    st, bloom, root, gas = core.ValidateReceipts(bad, [good[2][0]], [good[2][1]], [good[2][2]], ctx=ctx)
    assert st.tolist() == [R.ST_RECEIPT_STATUS] and not bloom.any() and not root.any() and gas.tolist() == [0]


def test_host_form_arguments(ctx):
    from gsv import GsvError, _lib, core
    st, bloom, root, gas = core.ValidateReceipts([], ctx=ctx)
    assert st.shape == (0,) and bloom.shape == (0, 256) and root.shape == (0, 32) and gas.shape == (0,)
    st, bloom, root, gas = core.ValidateReceipts([[], []], ctx=ctx)  # lists without a receipt
    assert st.tolist() == [0, 0] and not bloom.any() and gas.tolist() == [0, 0]
    assert root[0].tobytes() == root[1].tobytes() == R.EMPTY_ROOT
    with pytest.raises(ValueError):
        core.ValidateReceipts([[]], blooms=[bytes(255)], ctx=ctx)
    # a window into longer tables: voff and list_off need not start at 0
    lists = C.random_lists(31, [2, 3, 1])
    flat = b"\x99" * 7 + b"".join(b for lst in lists for b in lst)
    voff = np.cumsum([7] + [len(b) for lst in lists for b in lst]).astype(np.uint64)
    list_off = np.array([0, 2, 5, 6], np.uint64)
    L = _lib.load()
    import ctypes
    st = np.zeros(2, np.uint8)
    bloom = np.zeros((2, 256), np.uint8)
    root = np.zeros((2, 32), np.uint8)
    data = np.frombuffer(flat, np.uint8)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    rc = L.gsv_receipts_verify_batch(ctx.handle, p(data), p(voff), p(list_off[1:]), 2, None, None, None, None, p(bloom),
                                     p(root), None, p(st))
    assert rc == 0 and st.tolist() == [0, 0]
    e = expect(lists[1:])
    assert (bloom == e[1]).all() and (root == e[2]).all()
    rc = L.gsv_receipts_verify_batch(ctx.handle, p(data), p(voff), p(list_off), 3, None, None, None, None, None, None,
                                     None, None)
    assert rc == _lib.E_INVALID_ARG
    assert isinstance(GsvError("x", rc), RuntimeError)


# ---------------------------------------------------------------- 5. the _dev contract
class DevChain:
    """bloom -> DeriveSha -> check over torch tensors: the receipts behind an odd prefix at an odd address, every
    byte output in a guarded buffer at an odd offset"""

    def __init__(self, ctx, lists, prefix=3, want=None, receipt_rows=True):
        import torch
        import gsv
        self.ctx, self.lists = ctx, lists
        dev = self.dev = torch.device("cuda", ctx.device)
        blobs = [b for lst in lists for b in lst]
        self.n, self.nl = len(blobs), len(lists)
        self.bytes = sum(len(b) for b in blobs)
        self.voff = np.cumsum([prefix] + [len(b) for b in blobs]).astype(np.uint64)
        self.list_off = np.zeros(self.nl + 1, np.uint64)
        self.list_off[1:] = np.cumsum([len(lst) for lst in lists])
        z = lambda size, fill=0: torch.full((size,), fill, dtype=torch.uint8, device=dev)  # noqa: E731
        self.vals_buf = z(1 + prefix + self.bytes + 16, 0x99)
        self.vals = self.vals_buf[1:]
        self.load(blobs)
        self.d_voff = torch.from_numpy(self.voff.view(np.int64).copy()).to(dev)
        self.d_list_off = torch.from_numpy(self.list_off.view(np.int64).copy()).to(dev)
        self.work_bytes = gsv.receipts_work_bytes(self.n, self.bytes)
        self.work_buf = z(8 + self.work_bytes + 8, GUARD)
        self.gas_buf = z(8 + 8 * self.nl + 8, GUARD)
        self.width = {"rstatus": (self.n, 1), "rbloom": (self.n, 256), "lbloom": (self.nl, 256), "root": (self.nl, 32),
                      "lstatus": (self.nl, 1), "status": (self.nl, 1)}
        self.at = {"rstatus": 1, "rbloom": 3, "lbloom": 5, "root": 7, "lstatus": 9, "status": 11}
        self.bufs = {k: z(32 + r * w, GUARD) for k, (r, w) in self.width.items()}
        self.receipt_rows = receipt_rows
        self.want = None
        if want:
            wb, wr, wg = zip(*want)
            self.want = (z(1 + 256 * self.nl)[1:], z(1 + 32 * self.nl)[1:], torch.zeros(self.nl, dtype=torch.int64, device=dev))
            self.set_want(wb, wr, wg)

    def set_want(self, wb, wr, wg):
        import torch
        self.want[0].copy_(torch.from_numpy(np.frombuffer(b"".join(wb), np.uint8).copy()))
        self.want[1].copy_(torch.from_numpy(np.frombuffer(b"".join(wr), np.uint8).copy()))
        self.want[2].copy_(torch.from_numpy(np.array(wg, np.uint64).view(np.int64)))

    def load(self, blobs):
        import torch
        flat = np.frombuffer(b"".join(blobs), np.uint8).copy()
        at = int(self.voff[0])
        self.vals[at:at + flat.size].copy_(torch.from_numpy(flat))

    def view(self, k):
        r, w = self.width[k]
        return self.bufs[k][self.at[k]:self.at[k] + r * w]

    @property
    def work(self):
        return self.work_buf[8:8 + self.work_bytes]

    @property
    def gas(self):
        return self.gas_buf[8:8 + 8 * self.nl]

    def prepare(self):
        self.ctx.derive_sha_prepare(self.voff, self.list_off)

    def run(self, stream, vals_bytes=None, **k):
        a = dict(vals_t=self.vals, voff_t=self.d_voff, n_receipts=self.n, list_off_t=self.d_list_off, n_lists=self.nl,
                 vals_bytes=self.bytes if vals_bytes is None else vals_bytes, work_t=self.work,
                 receipt_status_t=self.view("rstatus"), receipt_bloom_t=self.view("rbloom") if self.receipt_rows else None,
                 list_bloom_t=self.view("lbloom"), gas_used_t=self.gas, list_status_t=self.view("lstatus"), stream=stream)
        a.update(k)
        self.ctx.receipts_bloom_dev(**a)
        self.ctx.derive_sha_batch_dev(self.vals, self.voff, self.list_off, self.view("root"), stream=stream, prepare=False)
        w = self.want or (None, None, None)
        self.ctx.receipts_check_dev(self.view("lstatus"), self.view("lbloom"), self.view("root"), self.gas, w[0], w[1], w[2],
                                    self.nl, self.view("status"), stream=stream)

    def get(self, k):
        """the rows of output k, after checking the guard bytes around them"""
        b = self.bufs[k].cpu().numpy()
        r, w = self.width[k]
        lo, hi = self.at[k], self.at[k] + r * w
        assert (b[:lo] == GUARD).all() and (b[hi:] == GUARD).all(), k
        return b[lo:hi].reshape(r, w) if w > 1 else b[lo:hi]

    def get_gas(self):
        g = self.gas_buf.cpu().numpy()
        assert (g[:8] == GUARD).all() and (g[-8:] == GUARD).all()
        w = self.work_buf.cpu().numpy()
        assert (w[:8] == GUARD).all() and (w[-8:] == GUARD).all(), "guard bytes around d_work"
        return g[8:-8].copy().view(np.uint64)

    def check(self, lists, want=None, receipt_rows=True):
        e = expect(lists, want)
        assert self.get("rstatus").tolist() == e[4]
        assert self.get("status").tolist() == e[0]
        assert self.get("lstatus").tolist() == [R.validate(lst)[0] for lst in lists]
        assert (self.get("lbloom") == e[1]).all() and (self.get("root") == e[2]).all()
        assert self.get_gas().tolist() == e[3]
        if receipt_rows:
            rows = [R.logs_bloom(R.decode_receipt(b)["logs"]) if R.decode_status(b)[0] == 0 else bytes(256)
                    for lst in lists for b in lst]
            assert (self.get("rbloom") == _rows(rows, 256)).all()
        assert (self.vals_buf.cpu().numpy()[:1 + int(self.voff[0])] == 0x99).all()
        return e


def test_dev_chain_contract(ctx):
    """odd voff[0], odd addresses of d_vals and every byte output, guard bytes, one launch per kernel id, the
    refusals, n == 0, and the chain captured into a graph and replayed once over changed receipts"""
    import torch
    from gsv import GsvError, _lib
    lists = C.random_lists(41, [3, 0, 70, 1, 9], max_logs=3)
    # failed receipts in the middle of a list: one without logs, and two whose logs are walked before the failure
    # shows (a bad status is judged behind the whole struct; a short topic behind the address and a good topic)
    lists[2][5] = C.raw(status=b"\x02")
    lists[2][9] = R.encode_receipt(R.new_receipt(status=b"\x02", gas=5, logs=[C.log(k, 3, b"late") for k in range(9)]))
    lists[2][11] = C.raw(logs=RLP.enc_list(R.encode_log(C.log(1, 2)) + C.raw_log(topics=RLP.enc_list(
        RLP.enc_string(C.topic(2)) + RLP.enc_string(bytes(31))))))
    assert [R.decode_status(lists[2][k])[0] for k in (5, 9, 11)] == [R.ST_RECEIPT_STATUS, R.ST_RECEIPT_STATUS, R.ST_BAD_RLP]
    lists[4][0] = R.encode_receipt(R.new_receipt(gas=9, logs=[C.log(k, k % 5) for k in range(40)]))
    e0 = expect(lists)
    want = [(bytes(e0[1][k]), bytes(e0[2][k]), e0[3][k]) for k in range(5)]
    want[0] = (want[0][0], want[0][1], want[0][2] + 1)       # gas
    want[3] = (want[3][0], bytes(32), want[3][2])            # root
    d = DevChain(ctx, lists, prefix=3, want=want)
    assert d.vals.data_ptr() % 2 == 1 and int(d.voff[0]) == 3
    for k in d.bufs:
        assert d.view(k).data_ptr() % 2 == 1, k
    d.prepare()
    torch.cuda.synchronize()
    (stream,) = ctx.pipeline_streams(1)
    try:
        ctx.set_timing(True)
        try:
            ctx.reset_timing()
            d.run(stream)
            stream.synchronize()
            for kid in (_lib.K_RECEIPT_SCAN, _lib.K_RECEIPT_BLOOM, _lib.K_RECEIPT_LISTS, _lib.K_RECEIPT_CHECK):
                ms, launches = ctx.kernel_time(kid)
                assert launches == 1 and ms > 0, kid
            # n == 0 enqueues nothing
            ctx.receipts_bloom_dev(None, None, 0, None, 0, 0, None, None, None, None, None, None, stream=stream)
            ctx.receipts_check_dev(None, None, None, None, None, None, None, 0, None, stream=stream)
            stream.synchronize()
            assert ctx.kernel_time(_lib.K_RECEIPT_SCAN)[1] == 1 and ctx.kernel_time(_lib.K_RECEIPT_CHECK)[1] == 1
        finally:
            ctx.set_timing(False)
            ctx.reset_timing()
        ex = d.check(lists, want)
        assert ex[0] == [R.ST_GAS_USED_MISMATCH, 0, R.ST_RECEIPT_STATUS, R.ST_INVALID_RECEIPT_ROOT, 0]

        def refused(**k):
            with pytest.raises(GsvError) as err:
                d.run(stream, **k)
            assert err.value.code == _lib.E_INVALID_ARG

        refused(work_t=d.work_buf[4:])                       # the work area off 8-byte alignment
        refused(gas_used_t=d.gas_buf[4:])
        refused(voff_t=d.d_voff.view(torch.uint8)[4:])
        refused(list_off_t=d.d_list_off.view(torch.uint8)[4:])
        refused(vals_t=None)
        refused(list_bloom_t=None)
        refused(vals_bytes=(1 << 40) + 1)
        stream.synchronize()
        d.check(lists, want)                                 # nothing was written by the refused calls

        # captured on a stream of the context's own, replayed once over changed receipts of the same lengths
        before = ctx.prepared_shapes()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            d.run(stream)
        assert ctx.prepared_shapes() == before
        changed = [list(lst) for lst in lists]
        r = R.decode_receipt(changed[0][1])
        r["logs"] = [(bytes(x ^ 0x5A for x in a), [bytes(x ^ 0xA5 for x in t) for t in ts], dt) for a, ts, dt in r["logs"]]
        r["status"] = b"\x01" if r["status"] == b"" else r["status"]
        changed[0][1] = R.encode_receipt(r)
        assert len(changed[0][1]) == len(lists[0][1])
        changed[2][5] = R.encode_receipt(R.decode_receipt(C.raw()))   # the failed receipt now decodes: same length
        assert len(changed[2][5]) == len(lists[2][5])
        assert changed[3][0][0] == 0xF9
        changed[3][0] = b"\xb9" + changed[3][0][1:]                   # a string where the receipt's list belongs
        d.load([b for lst in changed for b in lst])
        for buf in d.bufs.values():
            buf.fill_(GUARD)
        d.gas_buf.fill_(GUARD)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        ex = d.check(changed, want)
        assert ex[4][3 + 5] == R.ST_OK and ex[0][3] == R.ST_BAD_RLP  # list 2's receipt 5 is the batch's receipt 8
    finally:
        ctx.destroy_streams([stream])


def test_vals_bytes_one_receipt_too_small(ctx):
    """the caller's bound cuts the last receipt off: it is GSV_ST_BAD_RLP unread, nothing outside d_work is written
    for it, and every other receipt is served"""
    import torch
    lists = C.random_lists(51, [4, 6], max_logs=3)
    last = lists[1][-1]
    d = DevChain(ctx, lists, prefix=1, receipt_rows=False)
    d.prepare()
    (stream,) = ctx.pipeline_streams(1)
    try:
        for short in (d.bytes - len(last), d.bytes - 1):
            for buf in d.bufs.values():
                buf.fill_(GUARD)
            d.work_buf.fill_(GUARD)
            torch.cuda.synchronize()
            d.run(stream, vals_bytes=short)
            stream.synchronize()
            rst = d.get("rstatus").tolist()
            assert rst == [0] * 9 + [R.ST_BAD_RLP]
            assert d.get("status").tolist() == d.get("lstatus").tolist() == [0, R.ST_BAD_RLP]
            e = expect(lists[:1])
            assert (d.get("lbloom")[0] == e[1][0]).all() and not d.get("lbloom")[1].any()
            assert not d.get("root")[1].any() and d.get_gas().tolist() == [e[3][0], 0]
            assert (d.bufs["rbloom"].cpu().numpy() == GUARD).all()   # not asked for: untouched
    finally:
        ctx.destroy_streams([stream])
