"""GPU parity of the blob codec (csrc/blob.hip: k_blob_serialize, k_blob_strip, k_blob_unpack, with
notary.hip's k_blob_index) with the oracle's restatement of sharding/utils/marshal.go:71-198, byte for
byte, through the host forms and the device-resident forms.

The serialize kernel's launch constants (csrc/blob.hip): a lane stores BS_GROUP_BYTES = 16 bytes (half a
chunk), a wave BS_WAVE_BYTES = 1,024, a workgroup BS_BLOCK_BYTES = 4,096.  blob_corpus.straddle_lists()
holds blobs across each of those boundaries of the output."""
import numpy as np
import pytest

import blob_corpus as BC

pytestmark = pytest.mark.gpu

PAD = 256  # guard bytes around the output region (16-byte aligned)


def _tables(lists):
    blobs = [b for lst in lists for b, _ in lst]
    flags = np.array([f for lst in lists for _, f in lst] + [0], np.uint8)
    bo = np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)
    lo = np.cumsum([0] + [len(lst) for lst in lists]).astype(np.uint64)
    return np.frombuffer(b"".join(blobs) + b"\0", np.uint8)[:int(bo[-1])], bo, lo, flags[:len(blobs)]


def _oracle_bodies(oracle, lists):
    return [oracle.blob_serialize([b for b, _ in lst], [f for _, f in lst]) if lst else b"" for lst in lists]


@pytest.fixture(scope="module")
def batch(oracle):
    """one batch for the device-resident runs: five unequal lists (one 1-byte blob and an empty list between
    full ones) followed by the lists that straddle the kernel's boundaries; the oracle's bodies, once"""
    lists = BC.list_sets()["five lists"] + BC.straddle_lists()
    return lists, _oracle_bodies(oracle, lists)


def _dev_serialize(ctx, lists, align=0, end_on_4k=False, with_skip=True):
    """the _dev form with the input inside a larger 0xFF buffer, at `align` (0..3) past a 4-byte boundary
    or ending on a 4 KiB boundary, and the output inside a buffer of 0xA5: (bodies bytes, body_off)"""
    import torch
    import gsv
    dev = torch.device("cuda", ctx.device)
    flat, bo, lo, flags = _tables(lists)
    n = int(bo[-1])
    big = torch.full((n + 3 * 4096,), 0xFF, dtype=torch.uint8, device=dev)
    if end_on_4k:
        # offsets passed through blob_off (the batch then starts past d_blobs), the end on a page boundary
        shift = (-(big.data_ptr() + n)) % 4096 + 4096
        view, bo2 = big, bo + np.uint64(shift)
    else:
        shift = 16 + align
        view, bo2 = big[shift:], bo
    assert (big.data_ptr() + shift + n) % 4096 == 0 if end_on_4k else (big.data_ptr() + shift) % 4 == align
    big[shift:shift + n] = torch.from_numpy(flat.copy()).to(dev)
    body_off = gsv.blob_serialized_size(bo2, lo)
    total = int(body_off[-1])
    out = torch.full((total + 2 * PAD,), 0xA5, dtype=torch.uint8, device=dev)
    d_skip = torch.from_numpy(flags.copy()).to(dev) if with_skip and len(flags) else None
    cs = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    ctx.blob_serialize_batch_dev(view, bo2, lo, out[PAD:], d_skip, stream=cs)
    cs.synchronize()
    got = out.cpu().numpy()
    assert (got[:PAD] == 0xA5).all() and (got[PAD + total:] == 0xA5).all(), "a store left the output region"
    assert (big[:shift] == 0xFF).all() and (big[shift + n:] == 0xFF).all()
    return got[PAD:PAD + total].tobytes(), body_off


def _split(buf, off):
    return [buf[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


# ---------------------------------------------------------------- serialize
def test_serialize_host_form(ctx, oracle):
    sets = list(BC.list_sets().items()) + [("straddle", BC.straddle_lists())]
    for name, lists in sets:
        got = ctx.blob_serialize_batch([[b for b, _ in lst] for lst in lists], [[f for _, f in lst] for lst in lists])
        assert got == _oracle_bodies(oracle, lists), name
    # no flags: all false
    lists = BC.list_sets()["two lists"]
    got = ctx.blob_serialize_batch([[b for b, _ in lst] for lst in lists])
    assert got == [oracle.blob_serialize([b for b, _ in lst]) for lst in lists]


@pytest.mark.parametrize("n_lists", [1, 2, 5])
def test_serialize_dev_list_counts(ctx, oracle, batch, n_lists):
    lists = batch[0][:n_lists] if n_lists != 2 else [batch[0][0], batch[0][3]]
    buf, off = _dev_serialize(ctx, lists)
    assert _split(buf, off) == _oracle_bodies(oracle, lists)


@pytest.mark.parametrize("place", [0, 1, 2, 3, "4k"])
def test_serialize_dev_surroundings(ctx, batch, place):
    """the input at every base alignment inside 0xFF, its end on a 4 KiB boundary with 0xFF behind it, the
    output inside 0xA5: the same bytes as the oracle's, and nothing outside the output region written"""
    lists, want = batch
    if place == "4k":
        buf, off = _dev_serialize(ctx, lists, end_on_4k=True)
    else:
        buf, off = _dev_serialize(ctx, lists, align=place)
    assert _split(buf, off) == want


def test_serialize_dev_without_flags(ctx, oracle, batch):
    lists = batch[0][:4]
    buf, off = _dev_serialize(ctx, lists, align=1, with_skip=False)
    assert _split(buf, off) == [oracle.blob_serialize([b for b, _ in lst]) if lst else b"" for lst in lists]


def test_serialize_body_of_exactly_2_20_bytes(ctx, oracle):
    rng = np.random.default_rng(20)
    raw = rng.integers(1, 255, 8192 * 124, dtype=np.uint8).tobytes()
    lst = [(raw[124 * i:124 * (i + 1)], i & 1) for i in range(8192)]
    buf, off = _dev_serialize(ctx, [lst], align=3)
    assert list(off) == [0, 1 << 20]
    assert buf == oracle.blob_serialize([b for b, _ in lst], [f for _, f in lst])


def test_dev_calls_unprepared(ctx):
    import torch
    from gsv import GsvError, _lib
    dev = torch.device("cuda", ctx.device)
    bo = np.array([0, 77, 1234567], np.uint64)  # offsets no other test prepares
    lo = np.array([0, 2], np.uint64)
    t = torch.zeros((1 << 21,), dtype=torch.uint8, device=dev)
    with pytest.raises(GsvError) as e:
        ctx.blob_serialize_batch_dev(t, bo, lo, t, None, prepare=False)
    assert e.value.code == _lib.E_NOT_PREPARED
    h_off = np.array([0, 96 * 32 + 7], np.uint64)
    i32 = torch.zeros((64,), dtype=torch.int32, device=dev)
    with pytest.raises(GsvError) as e:
        ctx.blob_deserialize_batch_dev(t, h_off, 5, i32, i32, i32, t, t, prepare=False)
    assert e.value.code == _lib.E_NOT_PREPARED


# ---------------------------------------------------------------- deserialize
@pytest.fixture(scope="module")
def des_bodies(oracle, batch):
    """edge bodies (the notary test's: a trailing partial chunk, blobs that are no transactions, indicator
    bits 0x60; a body that ends in non-terminal chunks) and serialized lists; the oracle's blobs, once"""
    bodies = list(BC.edge_bodies().values()) + [b for b in batch[1]]
    return bodies, [oracle.blob_deserialize(b) for b in bodies]


def test_deserialize_host_form(ctx, des_bodies):
    bodies, want = des_bodies
    assert ctx.blob_deserialize_batch(bodies) == want
    assert ctx.blob_deserialize_batch([b"", b"\x01" * 31]) == [[], []]


def test_sharding_mirror_round_trip(ctx, oracle):
    from gsv import sharding
    lst = BC.list_sets()["two lists"][0]
    body = sharding.Serialize([b for b, _ in lst], [f for _, f in lst], ctx)
    assert body == oracle.blob_serialize([b for b, _ in lst], [f for _, f in lst])
    assert sharding.Deserialize(body, ctx) == [(b, f) for b, f in lst if b]  # zero-length blobs never come back
    txs = [b for b, _ in lst if b]
    assert sharding.DeserializeBlobToTx(sharding.SerializeTxToBlob(txs, ctx), ctx) == txs
    with pytest.raises(ValueError, match="the serialized body size 1048608 exceeded the collation size limit 1048576"):
        sharding.SerializeTxToBlob([bytes(124)] * 8192 + [b"\x01"], ctx)


@pytest.mark.parametrize("max_blobs", [3, 1024])
def test_deserialize_dev_form(ctx, des_bodies, max_blobs):
    """max_blobs below the blob count: nblobs reports the true count, only the first max_blobs rows are
    written; the data region holds every chunk's 31 bytes at 31 c, filler as it stands in the body"""
    import torch
    import gsv
    dev = torch.device("cuda", ctx.device)
    bodies, want = des_bodies
    n = len(bodies)
    lens = [len(b) for b in bodies]
    # bodies at unaligned offsets inside 0xFF
    h_off = np.cumsum([5] + lens).astype(np.uint64)
    flat = np.full(int(h_off[-1]) + 64, 0xFF, np.uint8)
    for i, b in enumerate(bodies):
        flat[int(h_off[i]):int(h_off[i + 1])] = np.frombuffer(b, np.uint8)
    d_bodies = torch.from_numpy(flat).to(dev)
    doff = gsv.blob_data_layout(h_off)
    d_n = torch.full((n,), -1, dtype=torch.int32, device=dev)
    d_s = torch.full((n + 1, max_blobs), -1, dtype=torch.int32, device=dev)
    d_l = torch.full((n + 1, max_blobs), -1, dtype=torch.int32, device=dev)
    d_k = torch.full((n + 1, max_blobs), 0xA5, dtype=torch.uint8, device=dev)
    d_d = torch.full((int(doff[-1]) + 2 * PAD,), 0xA5, dtype=torch.uint8, device=dev)
    cs = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    ctx.blob_deserialize_batch_dev(d_bodies, h_off, max_blobs, d_n, d_s, d_l, d_k, d_d[PAD:], stream=cs)
    cs.synchronize()
    nb, st, ln, sk, data = (x.cpu().numpy() for x in (d_n, d_s, d_l, d_k, d_d))
    assert (data[:PAD] == 0xA5).all() and (data[PAD + int(doff[-1]):] == 0xA5).all()
    assert (st[n] == -1).all() and (ln[n] == -1).all() and (sk[n] == 0xA5).all()  # the guard row
    data = data[PAD:]
    assert list(nb) == [len(w) for w in want]
    assert max(nb) > 3  # the small max_blobs cuts some body off
    for i, body in enumerate(bodies):
        nch = lens[i] // 32
        region = data[int(doff[i]):int(doff[i + 1])]
        stripped = b"".join(body[32 * c + 1:32 * c + 32] for c in range(nch))
        assert region[:31 * nch].tobytes() == stripped, i
        assert (region[31 * nch:] == 0).all(), i
        k = min(len(want[i]), max_blobs)
        for t in range(k):
            assert region[st[i, t]:st[i, t] + ln[i, t]].tobytes() == want[i][t][0], (i, t)
            assert sk[i, t] == want[i][t][1], (i, t)
        assert (st[i, k:] == 0).all() and (ln[i, k:] == 0).all() and (sk[i, k:] == 0).all(), i
