"""GPU tests of the batched SHA-256 and RIPEMD-160 kernels (csrc/hash_md.hip), of the sha256hash /
ripemd160hash / dataCopy precompiles and of RunPrecompiledContracts over a mixed batch.  SHA-256 is
checked against hashlib.sha256, RIPEMD-160 against tests/ripemd160_model.py (itself pinned to
tests/golden/md_hashes.json); a RIPEMD-160 row is the precompile's, 12 zero bytes and the digest.

Not here: a graph capture of the two _dev calls.  tests/test_gpu_stream_contract.py, whose way of
capturing the other _dev calls this file was to follow, captures none."""
import hashlib

import numpy as np
import pytest

import ripemd160_model as M
from conftest import golden

pytestmark = pytest.mark.gpu

KINDS = ["sha256", "ripemd160"]
_ref_cache = {}


def ref(kind, msg):
    """the 32-byte row of `msg`, computed once per message"""
    key = (kind, msg)
    if key not in _ref_cache:
        _ref_cache[key] = hashlib.sha256(msg).digest() if kind == "sha256" else M.precompile_row(msg)
    return _ref_cache[key]


def host(ctx, kind, msgs):
    return getattr(ctx, kind + "_batch")(msgs)


def dev(ctx, kind, data_t, off_t, out_t, stream=None):
    getattr(ctx, kind + "_batch_dev")(data_t, off_t, out_t, stream)


def rand_msgs(seed, lens):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in lens]


def bad_rows(kind, msgs, rows):
    return [(i, len(m)) for i, m in enumerate(msgs) if bytes(rows[i]) != ref(kind, m)][:10]


def offsets(msgs):
    off = np.zeros(len(msgs) + 1, np.int64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    return off


@pytest.mark.parametrize("kind", KINDS)
def test_fixture_vectors_and_the_empty_batch(ctx, kind):
    fx = golden("md_hashes.json")
    msgs = [r["msg"].encode() for r in fx["spec"] if "msg" in r]
    msgs += [M.long_message(r["long_message"]) if "long_message" in r else bytes.fromhex(r["msg"]) for r in fx["random"]]
    want = [r["ripemd160"] for r in fx["spec"] if "msg" in r] + [r["ripemd160"] for r in fx["random"]]
    assert len(msgs) == 8 + 41
    out = host(ctx, kind, msgs)
    assert out.shape == (len(msgs), 32) and out.dtype == np.uint8
    for i, m in enumerate(msgs):
        if kind == "ripemd160":  # the fixture's digests themselves, not the model's
            assert bytes(out[i]) == bytes(12) + bytes.fromhex(want[i]), (i, len(m))
        else:
            assert bytes(out[i]) == hashlib.sha256(m).digest(), (i, len(m))
    empty = host(ctx, kind, [])
    assert empty.shape == (0, 32)


@pytest.mark.parametrize("kind", KINDS)
def test_every_length_through_two_padding_blocks(ctx, kind):
    """0 .. 260 bytes in one batch: across 55/56, 63/64, 119/120 and 127/128, so one and two padding blocks
    behind zero to four message blocks, at whatever alignments the packed batch gives"""
    msgs = rand_msgs(11, range(261))
    assert not bad_rows(kind, msgs, host(ctx, kind, msgs))


@pytest.mark.parametrize("kind", KINDS)
def test_dev_form_at_every_start_alignment(ctx, kind):
    import torch
    msgs = rand_msgs(12, np.random.default_rng(120).integers(20, 201, 1500))
    flat = np.frombuffer(b"".join(msgs), np.uint8).copy()
    off_t = torch.from_numpy(offsets(msgs)).cuda()
    for shift in range(4):
        buf = torch.zeros(len(flat) + 16, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 4 == 0
        buf[shift:shift + len(flat)] = torch.from_numpy(flat).cuda()
        out = torch.zeros((len(msgs), 32), dtype=torch.uint8, device="cuda")
        dev(ctx, kind, buf[shift:shift + len(flat)], off_t, out)
        torch.cuda.synchronize()
        assert not bad_rows(kind, msgs, out.cpu().numpy()), shift


@pytest.mark.parametrize("kind", KINDS)
def test_block_count_buckets_in_one_batch(ctx, kind):
    """Messages are taken in block-count order inside each workgroup: a workgroup of one- to three-block
    messages, one long message among 255 short ones, 200 empty ones with a longer one still, and the
    lengths around the padding's block boundary; the last workgroup is partial"""
    lens = list(np.random.default_rng(130).integers(32, 129, 256))
    lens += [7] * 100 + [40000] + [30] * 155
    lens += [0] * 200 + [100000]
    for k in range(11):
        lens += [64 * k, 64 * k + 55, 64 * k + 56]
    assert len(lens) % 256 not in (0, 255) and len(lens) > 512
    msgs = rand_msgs(13, lens)
    assert not bad_rows(kind, msgs, host(ctx, kind, msgs))


@pytest.mark.parametrize("kind", KINDS)
def test_last_block_reads_at_batch_end(ctx, kind):
    """The batch ends on a 4 KiB boundary of its allocation with 0xff bytes after it, its last messages
    are 0 - 17 bytes long, and it starts at every alignment 0 - 3 (the layout of
    test_keccak256_tail_block_reads_at_batch_end): only dwords that hold a byte of a message are read,
    and the neighbours' bytes in them are masked"""
    import torch
    for shift in range(4):
        lens = [100 + shift] + list(np.random.default_rng(77).integers(100, 161, 700)) + list(range(18)) + [0, 0, 5]
        msgs = rand_msgs(14, lens)
        flat = np.frombuffer(b"".join(msgs), np.uint8).copy()
        buf = torch.full((len(flat) + 3 * 4096,), 0xff, dtype=torch.uint8, device="cuda")
        end = ((buf.data_ptr() + len(flat) + 4096) // 4096) * 4096 - buf.data_ptr()  # page-aligned end
        start = end - len(flat)
        assert 0 <= start and end + 16 <= buf.numel()
        buf[start:end] = torch.from_numpy(flat).cuda()
        out = torch.empty((len(msgs), 32), dtype=torch.uint8, device="cuda")
        dev(ctx, kind, buf[start:end], torch.from_numpy(offsets(msgs)).cuda(), out)
        torch.cuda.synchronize()
        assert not bad_rows(kind, msgs, out.cpu().numpy()), (buf.data_ptr() + start) % 4


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("out_shift", [1, 4, 8])
def test_unaligned_digest_output(ctx, kind, out_shift):
    """Rows to an output that is not 16-byte aligned go out as bytes; the bytes around it stay"""
    import torch
    msgs = rand_msgs(15 + out_shift, np.random.default_rng(150).integers(0, 200, 700))
    flat = np.frombuffer(b"".join(msgs), np.uint8).copy()
    data = torch.zeros(len(flat) + 64, dtype=torch.uint8, device="cuda")
    data[:len(flat)] = torch.from_numpy(flat).cuda()
    big = torch.full((len(msgs) * 32 + 32,), 0xee, dtype=torch.uint8, device="cuda")
    assert big.data_ptr() % 16 == 0
    out = big[out_shift:out_shift + len(msgs) * 32].view(len(msgs), 32)
    dev(ctx, kind, data, torch.from_numpy(offsets(msgs)).cuda(), out)
    torch.cuda.synchronize()
    b = big.cpu().numpy()
    assert (b[:out_shift] == 0xee).all() and (b[out_shift + len(msgs) * 32:] == 0xee).all()
    rows = b[out_shift:out_shift + len(msgs) * 32].reshape(len(msgs), 32)
    assert not bad_rows(kind, msgs, rows)
    if kind == "ripemd160":
        assert not rows[:, :12].any()


def test_precompile_semantics(ctx):
    from gsv import crypto, vm
    s, r, d = vm.Sha256Hash(), vm.Ripemd160Hash(), vm.DataCopy()
    assert s.Run(b"", ctx) == hashlib.sha256(b"").digest() and s.RequiredGas(b"") == 60
    assert r.Run(b"", ctx) == bytes(12) + bytes.fromhex("9c1185a5c5e9fc54612808977ee8f548b2258d31")
    assert r.RequiredGas(b"") == 600
    msg = bytes(range(100))
    assert s.Run(msg, ctx) == hashlib.sha256(msg).digest() and s.RequiredGas(msg) == 60 + 4 * 12
    assert r.Run(msg, ctx) == M.precompile_row(msg) and r.RequiredGas(msg) == 600 + 4 * 120
    assert d.Run(msg) == msg and d.RequiredGas(msg) == 15 + 4 * 3
    assert crypto.Sha256(b"abc", ctx) == hashlib.sha256(b"abc").digest()
    assert crypto.Ripemd160(b"abc", ctx).hex() == "8eb208f7e05d987a9b044a8e98c6b087f15a0bfc"
    both = crypto.Ripemd160Batch([b"abc", b""], ctx)
    assert both.shape == (2, 20) and bytes(both[1]).hex() == "9c1185a5c5e9fc54612808977ee8f548b2258d31"
    assert crypto.Sha256Batch([b"abc", msg], ctx).shape == (2, 32)
    assert vm.RunPrecompiledContract(r, b"", 600, ctx) == (r.Run(b"", ctx), None, 0)


def _mixed_items():
    """about 200 (address byte, input) from the existing fixtures, all eight addresses in turn"""
    bn, g1 = golden("bn256.json"), golden("bn256_g1.json")
    ec = []
    for c in golden("ecrecover.json")["cases"]:
        msg, sig = bytes.fromhex(c["msg"]), bytes.fromhex(c["sig"])
        if len(msg) == 32 and len(sig) == 65:  # hash || v || r || s (core/vm/contracts.go:82-87)
            ec.append(msg + bytes(31) + bytes([(sig[64] + 27) & 0xff]) + sig[:64])
    rng = np.random.default_rng(200)
    fam = {
        1: ec[:20] + [ec[0][:100], b""],
        2: rand_msgs(21, rng.integers(0, 300, 25)),
        3: rand_msgs(22, rng.integers(0, 300, 25)),
        4: rand_msgs(23, rng.integers(0, 100, 25)),
        5: [bytes.fromhex(v["input"]) for v in golden("modexp_vectors.json")["vectors"]] +
           [(2000).to_bytes(32, "big") * 3],  # lengths above the cap
        6: [bytes.fromhex(v["input"]) for v in g1["add"]] + [bytes.fromhex(v["input"]) for v in g1["generated"]["add"][:8]] +
           [b"\x01" * 128],
        7: [bytes.fromhex(v["input"]) for v in bn["scalar_mul"]] + [b"\x01" * 96],
        8: sorted((bytes.fromhex(v["input"]) for v in bn["pairing"] + bn["generated"]), key=len)[:12] + [bytes(191)],
    }
    return [(a, fam[a][k % len(fam[a])]) for k in range(25) for a in range(1, 9)]


def test_run_precompiled_contracts_over_a_mixed_batch(ctx):
    from gsv import vm
    C = vm.PrecompiledContractsByzantium
    items = _mixed_items()
    assert len(items) == 200 and {a for a, _ in items} == set(range(1, 9))
    addrs = [bytes(19) + bytes([a]) for a, _ in items]
    inputs = [x for _, x in items]
    need = [C[a].RequiredGas(x) for a, x in zip(addrs, inputs)]
    gas = [g - 1 if k % 7 == 6 else g + (k % 3) * 1000 for k, g in enumerate(need)]  # every 7th one gas short
    res = vm.RunPrecompiledContracts(C, addrs, inputs, gas, ctx=ctx)
    assert len(res) == len(items)
    single = {}  # per-item Run, once per distinct call
    for k, ((a, x), (ret, err, left)) in enumerate(zip(items, res)):
        if k % 7 == 6:
            assert ret is None and isinstance(err, vm.ErrOutOfGas) and left == gas[k], k
            continue
        if (a, x) not in single:
            try:
                one = C[addrs[k]].Run(x, ctx) if a != 4 else C[addrs[k]].Run(x)
                single[a, x] = (b"" if one is None else one, None)  # ecrecover's (nil, nil)
            except ValueError as e:
                single[a, x] = (None, type(e))
        want, werr = single[a, x]
        assert ret == want and (err is None if werr is None else type(err) is werr), (k, a)
        assert left == gas[k] - need[k], k
    kinds = {type(e) for _, e, _ in res if e is not None}
    assert {vm.ErrOutOfGas, vm.ErrModexpTooLong, vm.ErrMalformedPoint, vm.ErrBadPairingInput} <= kinds
    # the Homestead set has the first four only
    H = vm.PrecompiledContractsHomestead
    low = [k for k, (a, _) in enumerate(items) if a <= 4][:16]
    got = vm.RunPrecompiledContracts(H, [addrs[k] for k in low], [inputs[k] for k in low], [gas[k] for k in low], ctx=ctx)
    assert [(r, type(e)) for r, e, _ in got] == [(res[k][0], type(res[k][1])) for k in low]
    for a in range(5, 9):
        with pytest.raises(KeyError):
            vm.RunPrecompiledContracts(H, [addrs[0], bytes(19) + bytes([a])], [inputs[0], b""], [10**9] * 2, ctx=ctx)
