"""GPU tests of the bloombits family (include/gsv.h, "bloombits"): the section generator, the bitset codec, the matcher
and bloomFilter.  Expected values come from the model (tests/bloombits_model.py, pinned to the reference by
tests/test_bloombits_cpu.py) and the fixture (tests/golden/bloombits.json), never from the library."""
import random

import numpy as np
import pytest

import bloombits_model as M
import receipt_cases as C
import receipt_model as R
from conftest import golden

pytestmark = pytest.mark.gpu

GUARD = 0xEE
FX = golden("bloombits.json")


def _dev(ctx):
    import torch
    return torch.device("cuda", ctx.device)


def _put(ctx, a, lead=0, guard=0):
    """the bytes of `a` on the device `lead` bytes into an allocation, with `guard` guard bytes on both sides:
    (whole buffer, view of the payload)"""
    import torch
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = torch.full((lead + guard + a.size + guard + 8,), GUARD, dtype=torch.uint8, device=_dev(ctx))
    v = buf[lead + guard:lead + guard + a.size]
    if a.size:
        v.copy_(torch.from_numpy(a.copy()))
    return buf, v


def _guards_ok(buf, v):
    b = buf.cpu().numpy()
    lo = v.data_ptr() - buf.data_ptr()
    return (b[:lo] == GUARD).all() and (b[lo + v.numel():] == GUARD).all()


class Timed:
    """a stream of the context's own with kernel timing on; launches(kid) after a synchronize"""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        (self.stream,) = self.ctx.pipeline_streams(1)
        self.ctx.set_timing(True)
        self.ctx.reset_timing()
        return self

    def launches(self, kid):
        self.stream.synchronize()
        return self.ctx.kernel_time(kid)[1]

    def __exit__(self, *exc):
        self.stream.synchronize()
        self.ctx.set_timing(False)
        self.ctx.reset_timing()
        self.ctx.destroy_streams([self.stream])


# ---------------------------------------------------------------- 1. generator
def _blooms(seed, count):
    """half-density random blooms with an all-zero and an all-ones one among them"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (count, 256), dtype=np.uint8)
    a[1] = 0
    a[count - 2] = 0xFF
    return a


def _single_bits(count):
    """block j holds the single bloom bit 37 j mod 2048: an index slip moves it"""
    a = np.zeros((count, 256), np.uint8)
    for j in range(count):
        b = 37 * j % 2048
        a[j, 255 - b // 8] = 1 << (b % 8)
    return a


@pytest.mark.parametrize("n_sections", [1, 3])
@pytest.mark.parametrize("S", [8, 72, 2048, 4096])
def test_generator_host_form(ctx, S, n_sections):
    from gsv import bloombits
    for blooms in (_blooms(S + n_sections, S * n_sections), _single_bits(S * n_sections)):
        got = bloombits.GenerateSections(blooms, S, ctx)
        assert got.shape == (n_sections, 2048, S // 8) and got.dtype == np.uint8
        want = M.generate_sections_np(blooms, S)
        assert (got == want).all()
        if S <= 72:  # the model's own loop, statement for statement
            assert got.tobytes() == M.generate_sections([bytes(b) for b in blooms], S)
    one = _single_bits(S)
    t = bloombits.GenerateSections(one, S, ctx)[0]
    for j in range(0, S, max(1, S // 64)):
        assert t[37 * j % 2048, j // 8] & (1 << (7 - j % 8))
    assert int(np.unpackbits(t).sum()) == S


def test_generator_relation_of_the_reference(ctx):
    """TestGenerator at S = 2048: input i's bit j, MSB first, is output 2047 - j's bit i; through NewGenerator"""
    from gsv import bloombits
    blooms = _blooms(9, 2048)
    g = bloombits.NewGenerator(2048, ctx)
    for i in range(2048):
        g.AddBloom(i, blooms[i].tobytes())
    out = np.frombuffer(b"".join(g.Bitset(i) for i in range(2048)), np.uint8).reshape(2048, 256)
    a, b = np.unpackbits(blooms, axis=1), np.unpackbits(out, axis=1)
    assert (b[::-1].T == a).all()


@pytest.mark.parametrize("S,n_sections,in_lead,out_lead", [(72, 3, 1, 3), (8, 2, 3, 0), (4096, 1, 1, 0), (2048, 2, 0, 1),
                                                          (4096, 2, 0, 0), (520, 1, 0, 0)])
def test_generator_dev_form(ctx, S, n_sections, in_lead, out_lead):
    """input at an odd address, guard bytes on both sides of the table, one launch, nothing for no sections"""
    import torch
    from gsv import _lib
    blooms = _blooms(S, S * n_sections)
    blooms[0] = _single_bits(1)[0]
    _, d_in = _put(ctx, blooms, lead=in_lead)
    assert d_in.data_ptr() % 4 == in_lead
    size = n_sections * 2048 * (S // 8)
    buf = torch.full((out_lead + 16 + size + 16,), GUARD, dtype=torch.uint8, device=_dev(ctx))
    d_out = buf[out_lead + 16:out_lead + 16 + size]
    with Timed(ctx) as t:
        ctx.bloombits_generate_dev(d_in, n_sections, S, d_out, stream=t.stream)
        ctx.bloombits_generate_dev(None, 0, S, None, stream=t.stream)
        assert t.launches(_lib.K_BLOOMBITS_GENERATE) == 1
    assert _guards_ok(buf, d_out)
    assert d_out.cpu().numpy().tobytes() == M.generate_sections_np(blooms, S).tobytes()


def test_generator_takes_the_rows_of_the_receipt_path(ctx):
    """d_list_bloom256 of gsv_receipts_bloom_dev, one row per block, is the generator's input as it lies"""
    import torch
    import gsv
    lists = C.random_lists(61, [2, 0, 3, 1, 4, 1, 2, 5], max_logs=3)
    blobs = [b for lst in lists for b in lst]
    n, nl, nbytes = len(blobs), len(lists), sum(len(b) for b in blobs)
    dev = _dev(ctx)
    voff = np.cumsum([0] + [len(b) for b in blobs]).astype(np.int64)
    loff = np.cumsum([0] + [len(lst) for lst in lists]).astype(np.int64)
    _, vals = _put(ctx, np.frombuffer(b"".join(blobs), np.uint8))
    z = lambda k, dt=torch.uint8: torch.zeros(k, dtype=dt, device=dev)  # noqa: E731
    work, rst, lbloom, gas, lst_t = z(gsv.receipts_work_bytes(n, nbytes)), z(n), z(nl * 256), z(nl, torch.int64), z(nl)
    bits = z(2048)
    (stream,) = ctx.pipeline_streams(1)
    try:
        ctx.receipts_bloom_dev(vals, torch.from_numpy(voff).to(dev), n, torch.from_numpy(loff).to(dev), nl, nbytes, work,
                               rst, None, lbloom, gas, lst_t, stream=stream)
        ctx.bloombits_generate_dev(lbloom, 1, 8, bits, stream=stream)
        stream.synchronize()
    finally:
        ctx.destroy_streams([stream])
    want = [R.validate(lst)[1] for lst in lists]
    assert any(any(b) for b in want)
    assert bits.cpu().numpy().tobytes() == M.generate_sections(want, 8)


# ---------------------------------------------------------------- 2. compress
def _first_k(L, k, rng):
    return bytes(rng.randrange(1, 256) for _ in range(k)) + bytes(L - k)


def _grown(L):
    """vectors whose first k bytes are non-zero, k around the step where the model's length reaches L"""
    rng = random.Random(L)
    lo, hi = 0, L  # the model's length of k non-zero bytes in front is monotone in k: 0 at k = 0, L at k = L
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if len(M.compress_bytes(_first_k(L, mid, rng))) < L:
            lo = mid
        else:
            hi = mid
    return [_first_k(L, k, rng) for k in range(max(0, lo - 2), min(L, hi + 2) + 1)]


def _compress_vectors(L):
    rng = random.Random(100 + L)
    v = [bytes(L), bytes(rng.randrange(1, 256) for _ in range(L))]
    if L in (9, 512):
        v += [bytes(k) + bytes([1 + k % 255]) + bytes(L - 1 - k) for k in range(L)]
    v += _grown(L)
    v += [h for h in (bytes.fromhex(x) for x in FX["encoding_cycle"]) if len(h) == L]
    for dens in (0.5, 0.02, 0.2):
        v += [bytes(rng.randrange(1, 256) if rng.random() < dens else 0 for _ in range(L)) for _ in range(4)]
    return v


COMPRESS_LENGTHS = [1, 2, 9, 64, 512, 4096]


@pytest.fixture(scope="module")
def compressed():
    """per length: (vectors, the model's CompressBytes of each)"""
    out = {}
    for L in COMPRESS_LENGTHS + sorted({len(bytes.fromhex(x)) for x in FX["encoding_cycle"]}):
        if L not in out:
            vs = _compress_vectors(L)
            out[L] = (vs, [M.compress_bytes(x) for x in vs])
    return out


def test_compress_both_sides_of_the_step(compressed):
    """the batches hold a vector the model encodes to L - 1 bytes and one it stores raw, wherever L allows it"""
    for L in (9, 64, 512, 4096):
        lens = {len(c) for c in compressed[L][1]}
        assert {0, L - 1, L} <= lens, (L, sorted(lens)[-4:])
        enc = M.bitset_encode_bytes(compressed[L][0][1])
        assert len(enc) > L and compressed[L][1][1] == compressed[L][0][1]  # all non-zero: longer than the slot
    assert len(M.bitset_encode_bytes(compressed[512][0][1])) == 585


@pytest.mark.parametrize("L", COMPRESS_LENGTHS)
def test_compress_dev_form(ctx, compressed, L):
    """slots at an odd address, guard bytes around them, and nothing written behind a slot's length"""
    import torch
    from gsv import _lib
    vs, want = compressed[L]
    n = len(vs)
    _, d_in = _put(ctx, np.frombuffer(b"".join(vs), np.uint8), lead=1)
    sbuf = torch.full((3 + 16 + n * L + 16,), GUARD, dtype=torch.uint8, device=_dev(ctx))
    slots = sbuf[19:19 + n * L]
    lens = torch.full((n + 2,), -1, dtype=torch.int32, device=_dev(ctx))
    with Timed(ctx) as t:
        ctx.bitset_compress_batch_dev(d_in, n, L, slots, lens[1:n + 1], stream=t.stream)
        ctx.bitset_compress_batch_dev(None, 0, L, None, None, stream=t.stream)
        assert t.launches(_lib.K_BITSET_COMPRESS) == 1
    assert _guards_ok(sbuf, slots)
    ln = lens.cpu().numpy()
    assert ln[0] == -1 and ln[-1] == -1 and ln[1:-1].tolist() == [len(w) for w in want]
    s = slots.cpu().numpy().reshape(n, L)
    for i, w in enumerate(want):
        assert s[i, :len(w)].tobytes() == w, i
        assert (s[i, len(w):] == GUARD).all(), i


def test_compress_host_form_and_fixture(ctx, compressed):
    from gsv import bitutil
    for L, (vs, want) in compressed.items():
        assert bitutil.CompressBytesBatch(vs, ctx) == want, L
    for pair in FX["compression"]:
        assert bitutil.CompressBytes(bytes.fromhex(pair["in"]), ctx).hex() == pair["out"]
    assert bitutil.CompressBytesBatch([], ctx) == []


def test_compress_mixed_section(ctx):
    """2,048 vectors of 512 bytes with bit densities 0, 1/2, 1/4096 and 1/50 by row: empty, raw and encoded rows"""
    rng = np.random.default_rng(12)
    rows = np.zeros((2048, 512), np.uint8)
    for r in range(2048):
        dens = (0.0, 0.5, 1 / 4096, 1 / 50)[(r // 16) % 4]
        if dens:
            rows[r] = np.packbits(rng.random(4096) < dens)
    want = [M.compress_bytes(bytes(r)) for r in rows]
    kinds = {"empty": sum(len(w) == 0 for w in want), "raw": sum(len(w) == 512 for w in want)}
    kinds["encoded"] = 2048 - kinds["empty"] - kinds["raw"]
    assert all(kinds.values()), kinds
    got = ctx.bitset_compress_batch(rows)
    assert got == want
    out, st = ctx.bitset_decompress_batch(got, 512)
    assert not st.any() and (out == rows).all()


# ---------------------------------------------------------------- 3. decompress
def _crafted_512():
    """for L = 512 (levels 512, 64, 8, 1): one input per error that can occur at each level of the recursion, by the
    model.  errExceededTarget cannot occur inside the recursion at L = 512 (every level's bitset has exactly as many
    bits as its target); the inputs for it are of L = 9 and L = 100 below."""
    rng = random.Random(77)
    vec = bytes(rng.randrange(1, 256) if rng.random() < 0.3 else 0 for _ in range(512))
    enc = M.bitset_encode_bytes(vec)
    assert len(enc) < 512 and enc[0] != 0
    # the parts of the encoding: 1 byte, then the non-zero bytes of the levels of 8, 64 and 512
    l64 = bytes(sum((vec[8 * i + t] != 0) << (7 - t) for t in range(8)) for i in range(64))
    l8 = bytes(sum((l64[8 * i + t] != 0) << (7 - t) for t in range(8)) for i in range(8))
    n8, n64 = sum(b != 0 for b in l8), sum(b != 0 for b in l64)
    ends = {"8": 1 + n8, "64": 1 + n8 + n64, "512": len(enc)}
    out = {}
    for name, end in ends.items():
        start = {"8": 1, "64": ends["8"], "512": ends["64"]}[name]
        assert end - start >= 2
        out["missing data at level " + name] = (enc[:end - 1], M.ST_MISSING_DATA)
        z = bytearray(enc)
        z[start + 1] = 0
        out["zero content at level " + name] = (bytes(z), M.ST_ZERO_CONTENT)
    out["unreferenced data"] = (enc + b"\x01", M.ST_UNREFERENCED_DATA)
    out["zero first byte"] = (b"\x00" + enc[1:], M.ST_UNREFERENCED_DATA)
    # an inner level's error comes before an outer one's: zero content at level 8 and missing data at level 512
    z = bytearray(enc[:-1])
    z[2] = 0
    out["inner first"] = (bytes(z), M.ST_ZERO_CONTENT)
    # inside a level per bit: missing data before zero content
    z = bytearray(enc[:ends["64"] + 3])
    z[ends["64"] + 1] = 0
    out["order inside a level"] = (bytes(z), M.ST_ZERO_CONTENT)
    out["valid"] = (enc, M.ST_OK)
    return out


def test_crafted_inputs_mean_what_they_say():
    for name, (data, want) in _crafted_512().items():
        assert M.decompress_bytes(data, 512)[1] == want, name
    # errExceededTarget inside the recursion: a bit past the target of the level of 2 (L = 9), of 9, and of 100
    assert M.decompress_bytes(b"\x20\x01", 9)[1] == M.ST_EXCEEDED_TARGET        # level of 2: bit 2
    assert M.decompress_bytes(b"\x40\x01\x05", 9)[1] == M.ST_EXCEEDED_TARGET    # level of 9: bit 15 of two bytes
    assert M.decompress_bytes(b"\x40\x08\x01\x05", 100)[1] == M.ST_EXCEEDED_TARGET  # level of 100: bit 103


def _decompress_cases(compressed):
    """(target, inputs) per target length"""
    cases = {L: list(want) for L, (_, want) in compressed.items()}
    for name, (data, _) in _crafted_512().items():
        cases[512].append(data)
    cases[9] += [b"\x20\x01", b"\x40\x01\x05", b"\xc0\x01\x01\x01\x01\x01\x01\x01\x01\x01", b"\x01" * 9, b""]
    cases.setdefault(100, []).extend([b"\x40\x08\x01\x05", bytes(100), b"\x07" * 101, b""])
    cases[512] += [b"\x01" * 513, b"\x00" * 512, b"\x01" * 512, b"", b"\x00", b"\x80", b"\x80\x80", b"\x80\x80\x80"]
    cases.setdefault(2, []).append(bytes.fromhex(FX["compression_long"]["input"]))
    for row in FX["decoding_cycle"]:
        if 0 < row["size"] <= 4096:
            cases.setdefault(row["size"], []).append(bytes.fromhex(row["input"]))
    return cases


def test_decompress_against_the_model(ctx, compressed):
    """every compress output round-trips; the fixture's rows of size <= 4,096; the crafted errors; inputs longer than
    and as long as the target.  Statuses as the model's DecompressBytes, failed rows zero."""
    from gsv import bitutil
    cases = _decompress_cases(compressed)
    assert {1, 2, 9, 52, 64, 100, 512, 1024, 4096} <= set(cases)
    seen = set()
    for L, items in sorted(cases.items()):
        rows, st = bitutil.DecompressBytesBatch(items, L, ctx)
        assert rows.shape == (len(items), L)
        for i, x in enumerate(items):
            want, wst = M.decompress_bytes(x, L)
            assert st[i] == wst, (L, i, x[:16].hex())
            assert rows[i].tobytes() == (want if wst == M.ST_OK else bytes(L)), (L, i)
            seen.add(wst)
    assert seen == {M.ST_OK, M.ST_MISSING_DATA, M.ST_UNREFERENCED_DATA, M.ST_EXCEEDED_TARGET, M.ST_ZERO_CONTENT}
    for L, (vs, want) in compressed.items():
        for v, w in list(zip(vs, want))[:6]:
            assert bitutil.DecompressBytes(w, L, ctx) == v
    with pytest.raises(bitutil.ErrExceededTarget):
        bitutil.DecompressBytes(bytes.fromhex("c00101"), 2, ctx)
    with pytest.raises(bitutil.ErrZeroContent):
        bitutil.DecompressBytes(bytes.fromhex("8000"), 1024, ctx)
    # the fixture's sizes of 0 are the wrapper's, by DecompressBytes' own rule (a longer input exceeds the target)
    rows, st = bitutil.DecompressBytesBatch([b"", b"\x30"], 0, ctx)
    assert st.tolist() == [M.decompress_bytes(b"", 0)[1], M.decompress_bytes(b"\x30", 0)[1]] == [0, M.ST_EXCEEDED_TARGET]


def test_decompress_dev_form(ctx, compressed):
    """a table that does not start at 0, data and rows at odd addresses, guard bytes, one launch"""
    import torch
    from gsv import _lib
    items = _decompress_cases(compressed)[512]
    n, L = len(items), 512
    off = np.cumsum([5] + [len(x) for x in items]).astype(np.int64)
    _, data = _put(ctx, np.frombuffer(b"\x99" * 5 + b"".join(items), np.uint8), lead=1)
    obuf = torch.full((1 + 16 + n * L + 16,), GUARD, dtype=torch.uint8, device=_dev(ctx))
    out = obuf[17:17 + n * L]
    sbuf = torch.full((8 + n + 8,), GUARD, dtype=torch.uint8, device=_dev(ctx))
    with Timed(ctx) as t:
        ctx.bitset_decompress_batch_dev(data, torch.from_numpy(off).to(_dev(ctx)), n, L, out, sbuf[8:8 + n], stream=t.stream)
        ctx.bitset_decompress_batch_dev(None, None, 0, L, None, None, stream=t.stream)
        assert t.launches(_lib.K_BITSET_DECOMPRESS) == 1
    assert _guards_ok(obuf, out) and _guards_ok(sbuf, sbuf[8:8 + n])
    rows, st = out.cpu().numpy().reshape(n, L), sbuf.cpu().numpy()[8:8 + n]
    for i, x in enumerate(items):
        want, wst = M.decompress_bytes(x, L)
        assert st[i] == wst and rows[i].tobytes() == (want if wst == M.ST_OK else bytes(L)), i


# ---------------------------------------------------------------- 4. matcher
class DevQueries:
    """queries as lists of rules of clauses of three bit numbers, in the device layout"""

    def __init__(self, ctx, queries, ranges):
        import torch
        dev = _dev(ctx)
        cl, ro, qo = [], [0], [0]
        for rules in queries:
            for rule in rules:
                cl += [list(c) for c in rule]
                ro.append(len(cl))
            qo.append(len(ro) - 1)
        self.n_clauses, self.n_rules, self.n_queries = len(cl), len(ro) - 1, len(queries)
        arr = np.array(cl, np.uint16).reshape(-1, 3).view(np.int16)
        self.clauses = torch.from_numpy(arr.copy()).to(dev) if len(cl) else torch.zeros((1, 3), dtype=torch.int16, device=dev)
        self.rule_off = torch.tensor(ro, dtype=torch.int32, device=dev)
        self.query_off = torch.tensor(qo, dtype=torch.int32, device=dev)
        self.begin = torch.tensor([b for b, _ in ranges], dtype=torch.int64, device=dev)
        self.end = torch.tensor([e for _, e in ranges], dtype=torch.int64, device=dev)


def run_match(ctx, table, S, first, n_sections, dq, stream, lead=0, capacity=None):
    """match_dev then blocks_dev over guarded buffers: (bitsets (q, s, S / 8), counts (q, s), block_off, blocks)"""
    import torch
    dev = _dev(ctx)
    nq, rb = dq.n_queries, S // 8
    _, bits = _put(ctx, table, lead=lead)
    mbuf = torch.full((lead + 16 + nq * n_sections * rb + 16,), GUARD, dtype=torch.uint8, device=dev)
    match = mbuf[lead + 16:lead + 16 + nq * n_sections * rb]
    cbuf = torch.full((nq * n_sections + 2,), -1, dtype=torch.int32, device=dev)
    ctx.bloombits_match_dev(bits, S, first, n_sections, dq.clauses, dq.n_clauses, dq.rule_off, dq.n_rules, dq.query_off,
                            nq, dq.begin, dq.end, match, cbuf[1:-1], stream=stream)
    stream.synchronize()
    counts = cbuf.cpu().numpy()
    assert counts[0] == -1 and counts[-1] == -1 and _guards_ok(mbuf, match)
    total = int(counts[1:-1].sum())
    cap = total if capacity is None else capacity
    obuf = torch.full((nq + 3,), -1, dtype=torch.int64, device=dev)
    bbuf = torch.full((cap + 2,), -1, dtype=torch.int64, device=dev)
    ctx.bloombits_blocks_dev(match, cbuf[1:-1], S, first, n_sections, nq, obuf[1:nq + 2], bbuf[1:cap + 1], cap,
                             stream=stream)
    stream.synchronize()
    o, b = obuf.cpu().numpy(), bbuf.cpu().numpy()
    assert o[0] == -1 and o[-1] == -1 and b[0] == -1 and b[-1] == -1
    return (match.cpu().numpy().reshape(nq, n_sections, rb), counts[1:-1].reshape(nq, n_sections), o[1:-1], b[1:-1])


def check_match(got, queries, ranges, rows, S, first, n_sections, capacity=None):
    bitsets, counts, block_off, blocks = got
    want_all = []
    for q, (f, (b, e)) in enumerate(zip(queries, ranges)):
        for s in range(n_sections):
            wb, wc = M.match_bitset(f, lambda bit, k=first + s: rows(k, bit), S, first + s, b, e)
            assert bitsets[q, s].tobytes() == wb and counts[q, s] == wc, (q, s)
        want = M.match_blocks(f, rows, S, first, n_sections, b, e)
        assert block_off[q] == len(want_all) and block_off[q + 1] == len(want_all) + len(want), q
        want_all += want
    cap = len(want_all) if capacity is None else capacity
    assert blocks[:cap].tolist() == want_all[:cap]
    return want_all


@pytest.fixture(scope="module")
def modulo_case():
    """S = 4096, 3 sections, rows block % bit == 0 (matcher_test.go:247-259); the reference's filters and the edge
    ranges, filled up to 76 queries"""
    S, ns = FX["matcher"]["section_size"], 3
    rng = random.Random(31)
    queries, ranges = [], []
    for case in FX["matcher"]["continuous"] + [FX["matcher"]["shifted"]]:
        queries.append(case["filter"])
        ranges.append((case["start"], case["blocks"] - 1))
    f0 = queries[0]
    extra = [([], (100, 200)), ([], (0, S * ns + 50)), (f0, (4098, 4101)), (f0, (60, 60)), (f0, (61, 61)),
             (f0, (20000, 30000)), (f0, (500, 100)), (f0, (4095, 4096)), ([], (8191, 8192)), (f0, (0, 0)),
             ([[[2, 3, 5], [2048 + 7, 4096 + 11, 13]]], (1, 12000))]
    for f, r in extra:
        queries.append(f)
        ranges.append(r)
    while len(queries) < 76:
        queries.append([[[rng.randrange(2, 21) for _ in range(3)] for _ in range(rng.randrange(1, 4))]
                        for _ in range(rng.randrange(1, 4))])
        b = rng.randrange(0, S * ns)
        ranges.append((b, b + rng.choice((0, 5, 300, 5000, 20000))))
    bits = sorted({b & 2047 for f in queries for rule in f for cl in rule for b in cl})
    table = np.zeros((ns, 2048, S // 8), np.uint8)
    for s in range(ns):
        for b in bits:
            table[s, b] = np.frombuffer(M.modulo_row(b, s, S), np.uint8)
    return S, ns, queries, ranges, table


def test_matcher_modulo_rows(ctx, modulo_case):
    from gsv import _lib
    S, ns, queries, ranges, table = modulo_case
    rows = lambda s, bit: table[s, bit].tobytes()  # noqa: E731
    dq = DevQueries(ctx, queries, ranges)
    with Timed(ctx) as t:
        got = run_match(ctx, table, S, 0, ns, dq, t.stream)
        for kid in (_lib.K_BLOOMBITS_MATCH, _lib.K_BLOOMBITS_TOTALS, _lib.K_BLOOMBITS_SCAN, _lib.K_BLOOMBITS_BLOCKS):
            assert t.launches(kid) == 1, kid
        want = check_match(got, queries, ranges, rows, S, 0, ns)
        # the reference's expectation, for its own cases
        for q in range(3):
            lo, hi = ranges[q]
            assert got[3][got[2][q]:got[2][q + 1]].tolist() == [i for i in range(lo, min(hi, S * ns - 1) + 1)
                                                               if M.exp_match3(queries[q], i)]
        assert got[3][got[2][2]:got[2][3]].tolist() == [16, 32, 48]
        # a capacity below the total: true totals, nothing past the capacity
        cap = len(want) // 3
        short = run_match(ctx, table, S, 0, ns, dq, t.stream, capacity=cap)
        assert short[2].tolist() == got[2].tolist() and short[2][-1] == len(want) > cap
        assert short[3].tolist() == want[:cap]
        none = run_match(ctx, table, S, 0, ns, dq, t.stream, capacity=0)
        assert none[2].tolist() == got[2].tolist()
        # no queries, no sections: nothing enqueued
        ctx.reset_timing()
        ctx.bloombits_match_dev(None, S, 0, ns, None, 0, None, 0, None, 0, None, None, None, None, stream=t.stream)
        ctx.bloombits_blocks_dev(None, None, S, 0, ns, 0, None, None, 0, stream=t.stream)
        assert t.launches(_lib.K_BLOOMBITS_MATCH) == 0 and t.launches(_lib.K_BLOOMBITS_SCAN) == 0


@pytest.mark.parametrize("S,ns,first,lead", [(8, 5, 3, 1), (72, 4, 1000, 1), (72, 2, 0, 0), (32768, 1, 2, 0)])
def test_matcher_small_and_odd_sections(ctx, S, ns, first, lead):
    """rows that are no whole number of words, tables and bitsets at odd addresses, a table that starts at a section
    other than 0, bit numbers above 11 bits"""
    rng = random.Random(S + ns)
    nprng = np.random.default_rng(S)
    table = np.zeros((ns, 2048, S // 8), np.uint8)
    used = [3, 77, 500, 1024, 2047, 0, 9]
    for b in used:
        table[:, b] = np.packbits(nprng.random((ns, S)) < 0.7, axis=1)
    rows = lambda s, bit: table[s - first, bit].tobytes()  # noqa: E731
    queries, ranges = [[]], [(first * S + 1, (first + ns) * S - 2)]
    for _ in range(20):
        queries.append([[[rng.choice(used) + rng.choice((0, 2048, 63488)) for _ in range(3)]
                         for _ in range(rng.randrange(1, 3))] for _ in range(rng.randrange(1, 3))])
        b = first * S + rng.randrange(-S // 2, ns * S)
        ranges.append((max(0, b), max(0, b) + rng.choice((0, 1, 7, 8, 9, S, 3 * S))))
    dq = DevQueries(ctx, queries, ranges)
    with Timed(ctx) as t:
        got = run_match(ctx, table, S, first, ns, dq, t.stream, lead=lead)
    want = check_match(got, queries, ranges, rows, S, first, ns)
    assert len(want) > ns * S // 2


def _sparse_blooms(seed, count, pool):
    """blocks whose bloom is LogsBloom of a few items of a pool: (blooms (count, 256), the items of each block)"""
    rng = random.Random(seed)
    blooms, held = np.zeros((count, 256), np.uint8), []
    for j in range(count):
        items = rng.sample(pool, rng.randrange(0, 4))
        acc = 0
        for it in items:
            acc |= R.bloom9(it)
        blooms[j] = np.frombuffer(R.to_bloom(acc), np.uint8)
        held.append(items)
    return blooms, held


def test_matcher_host_form_with_the_reference_wildcards(ctx):
    """TestMatcherWildcards' filter through NewMatcher and Matches over a generated table"""
    from gsv import bloombits
    w = FX["wildcards"]
    filters = [None if rule is None else [None if cl is None else bytes.fromhex(cl) for cl in rule] for rule in w["filters"]]
    m = bloombits.NewMatcher(72, filters, ctx)
    assert [len(r) for r in m.filters] == w["kept"]
    assert m.filters == M.new_matcher_filters(filters)
    pool = [bytes.fromhex(cl) for rule in w["filters"][:3] for cl in rule] + [b"\x07" * 20, b"\x09" * 32]
    blooms, _ = _sparse_blooms(3, 72 * 3, pool)
    table = bloombits.GenerateSections(blooms, 72, ctx)
    assert table.tobytes() == M.generate_sections_np(blooms, 72).tobytes()
    bits = M.new_matcher_filters(filters)
    for first, begin, end in ((0, 0, 215), (5, 5 * 72 + 3, 5 * 72 + 150), (0, 300, 400)):
        want = [first * 72 + j for j in range(216) if M.filter_bits(bits, bytes(blooms[j])) and begin <= first * 72 + j <= end]
        got = m.Matches(table, first, begin, end)
        assert got.dtype == np.uint64 and got.tolist() == want
    assert len(m.Matches(table, 0, 0, 215)) > 0
    # all rules dropped: the wildcard; and several filters in one call, one of them short of capacity at first
    assert bloombits.NewMatcher(72, [[None], []], ctx).Matches(table, 0, 10, 20).tolist() == list(range(10, 21))
    many = bloombits.MatchBatch(72, table, 0, [filters, None, [[pool[0]]]], [0, 0, 0], [215, 215, 100], ctx)
    assert many[0].tolist() == m.Matches(table, 0, 0, 215).tolist() and many[1].tolist() == list(range(216))
    assert many[2].tolist() == [j for j in range(101) if M.filter_bits([[M.bloom_indexes(pool[0])]], bytes(blooms[j]))]
    few = ctx.bloombits_match_batch(table, 72, 0, [None], [0], [215], capacity=10)
    assert few[0].tolist() == list(range(10))


def test_matcher_equals_bloom_filter_over_a_generated_table(ctx):
    """the matcher's blocks over a table made by the generator from random sparse blooms are the blocks whose bloom
    passes gsv_bloom_filter_dev, and both are the model's; the clauses are hashed on the device by bloom9_batch_dev"""
    import torch
    from gsv import _lib, filters as F
    S, ns = 2048, 2
    pool = [bytes([k]) * 20 for k in range(1, 9)] + [bytes([k]) * 32 for k in range(1, 13)]
    blooms, _ = _sparse_blooms(8, S * ns, pool)
    specs = [([pool[0]], []), ([], [[pool[9]]]), ([pool[1], pool[2]], [[pool[10], pool[11]], [], [pool[12]]]),
             ([], []), ([b"\xaa" * 20], []), ([], [[pool[8]], [pool[9]], [pool[10]]]), (pool[:8], [pool[8:]])]
    flat = [M.flatten(a, t) for a, t in specs]
    kept = [M.kept_rules(f) for f in flat]
    # the kept clauses hashed on the device: bloom9_batch_dev's rows are the match call's clauses as they lie
    clauses = [cl for f in kept for rule in f for cl in rule]
    off = np.cumsum([0] + [len(c) for c in clauses]).astype(np.int64)
    dev = _dev(ctx)
    _, data = _put(ctx, np.frombuffer(b"".join(clauses), np.uint8))
    idx = torch.zeros((len(clauses), 3), dtype=torch.int16, device=dev)
    dq = DevQueries(ctx, [[[[0, 0, 0]] * len(rule) for rule in f] for f in kept], [(0, S * ns - 1)] * len(specs))
    _, d_blooms = _put(ctx, blooms, lead=1)
    table = torch.zeros(ns * 2048 * (S // 8), dtype=torch.uint8, device=dev)
    verdict = torch.full((len(specs) * S * ns + 16,), GUARD, dtype=torch.uint8, device=dev)
    with Timed(ctx) as t:
        ctx.bloom9_batch_dev(data, torch.from_numpy(off).to(dev), idx, stream=t.stream)
        dq.clauses = idx
        ctx.bloombits_generate_dev(d_blooms, ns, S, table, stream=t.stream)
        ctx.bloom_filter_dev(d_blooms, S * ns, dq.clauses, dq.n_clauses, dq.rule_off, dq.n_rules, dq.query_off,
                             dq.n_queries, verdict[8:8 + len(specs) * S * ns], stream=t.stream)
        ctx.bloom_filter_dev(None, 0, None, 0, None, 0, dq.query_off, dq.n_queries, None, stream=t.stream)
        assert t.launches(_lib.K_BLOOM_FILTER) == 1
        made = table.cpu().numpy().reshape(ns, 2048, S // 8)
        assert (made == M.generate_sections_np(blooms, S)).all()
        got = run_match(ctx, made, S, 0, ns, dq, t.stream)
    v = verdict.cpu().numpy()
    assert (v[:8] == GUARD).all() and (v[8 + len(specs) * S * ns:] == GUARD).all()
    v = v[8:8 + len(specs) * S * ns].reshape(len(specs), S * ns)
    assert set(np.unique(v)) <= {0, 1}
    hits = 0
    for q, (a, tp) in enumerate(specs):
        want = [j for j in range(S * ns) if M.bloom_filter(bytes(blooms[j]), a, tp)]
        assert np.flatnonzero(v[q]).tolist() == want, q
        assert got[3][got[2][q]:got[2][q + 1]].tolist() == want, q
        hits += 0 < len(want) < S * ns
        # the public call
        if q < 3:
            assert np.flatnonzero(F.BloomFilter(blooms[:300], a, tp, ctx)).tolist() == [j for j in want if j < 300]
    assert hits >= 3 and got[2][4] == got[2][3] + S * ns  # the wildcard matches every block


# ---------------------------------------------------------------- 5. capture
def test_generate_match_blocks_in_one_graph(ctx):
    """generate_dev -> match_dev -> blocks_dev captured on a stream of the context's own and replayed twice, the
    second time over other blooms"""
    import torch
    S, ns, first = 72, 3, 4
    pool = [bytes([k]) * 32 for k in range(1, 7)]
    sets = [_sparse_blooms(seed, S * ns, pool)[0] for seed in (1, 2)]
    bits = [[M.bloom_indexes(pool[0])], [M.bloom_indexes(pool[1]), M.bloom_indexes(pool[2])]]
    queries = [[bits[0]], [bits[1]], bits, []]
    ranges = [(0, 10 ** 6), (first * S + 5, first * S + 150), (first * S, (first + ns) * S - 1), (first * S + 70, first * S + 75)]
    dq = DevQueries(ctx, queries, ranges)
    dev = _dev(ctx)
    nq, rb = len(queries), S // 8
    _, d_blooms = _put(ctx, sets[0], lead=1)
    table = torch.zeros(ns * 2048 * rb, dtype=torch.uint8, device=dev)
    match = torch.zeros(nq * ns * rb, dtype=torch.uint8, device=dev)
    count = torch.zeros(nq * ns, dtype=torch.int32, device=dev)
    block_off = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    cap = 700
    blocks = torch.zeros(cap, dtype=torch.int64, device=dev)

    def chain(stream):
        ctx.bloombits_generate_dev(d_blooms, ns, S, table, stream=stream)
        ctx.bloombits_match_dev(table, S, first, ns, dq.clauses, dq.n_clauses, dq.rule_off, dq.n_rules, dq.query_off, nq,
                                dq.begin, dq.end, match, count, stream=stream)
        ctx.bloombits_blocks_dev(match, count, S, first, ns, nq, block_off, blocks, cap, stream=stream)

    def expect(blooms):
        t = M.generate_sections_np(blooms, S)
        rows = lambda s, bit: t[s - first, bit].tobytes()  # noqa: E731
        out = [M.match_blocks(f, rows, S, first, ns, b, e) for f, (b, e) in zip(queries, ranges)]
        return out

    def check(blooms):
        want = expect(blooms)
        off = block_off.cpu().numpy().tolist()
        assert off == np.cumsum([0] + [len(w) for w in want]).tolist()
        assert off[-1] <= cap and blocks.cpu().numpy()[:off[-1]].tolist() == [b for w in want for b in w]
        return want
    (stream,) = ctx.pipeline_streams(1)
    try:
        chain(stream)
        stream.synchronize()
        check(sets[0])
        before = ctx.prepared_shapes()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            chain(stream)
        assert ctx.prepared_shapes() == before
        for k in (0, 1):
            d_blooms.copy_(torch.from_numpy(sets[k].reshape(-1).copy()))
            for t in (table, match, blocks):
                t.fill_(0x55)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            want = check(sets[k])
            assert want[3] == list(range(first * S + 70, first * S + 76)) and len(want[0]) > 0
        assert expect(sets[0]) != expect(sets[1])
    finally:
        ctx.destroy_streams([stream])
