"""The batched modexp precompile on the GPU against the reference's vectors (tests/golden/modexp_vectors.json)
and the model (tests/modexp_model.py) over tests/modexp_corpus.py: the host form, the mirror class, mixed waves,
and the device-resident form on a stream of the context's with guarded buffers."""
import random

import numpy as np
import pytest

import modexp_corpus as C
import modexp_model as M
from conftest import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vectors():
    return [(v["name"], bytes.fromhex(v["input"]), bytes.fromhex(v["expected"]))
            for v in golden("modexp_vectors.json")["vectors"]]


# ---------------------------------------------------------------- (a) the reference's vectors
def test_reference_vectors(ctx, vectors):
    from gsv import _lib, vm
    assert len(vectors) == 17
    outs, st = ctx.modexp_batch([inp for _, inp, _ in vectors])
    assert (st == _lib.ST_OK).all()
    for (name, _, exp), got in zip(vectors, outs):
        assert got == exp, name
    pc = vm.BigModExp()
    for name, inp, exp in vectors:
        assert pc.Run(inp, ctx) == exp, name
    with pytest.raises(vm.ErrModexpTooLong):
        pc.Run(C.word(1) + C.word(1025) + C.word(1) + b"\x02", ctx)
    assert pc.Run(b"", ctx) == b""


# ---------------------------------------------------------------- (b) the corpus in one call
def test_corpus_in_one_call(ctx):
    import ctypes
    from gsv import _lib, _pack, _ptr
    inputs = [b for _, b in C.items()]
    labels = [l for l, _ in C.items()]
    want = [M.run_capped(b) for b in inputs]
    n = len(inputs)
    flat, off = _pack(inputs)
    out_off = np.zeros(n + 1, np.uint64)
    st = np.full(n, 0xEE, np.uint8)
    L = _lib.load()
    assert L.gsv_modexp_output_layout(_ptr(flat), _ptr(off), n, _ptr(out_off), _ptr(st)) == 0
    lens = [len(o) for _, o in want]
    assert list(np.diff(out_off.astype(np.int64))) == lens and int(out_off[n]) == sum(lens)
    assert list(st) == [s for s, _ in want]
    flat0, off0, out_off0 = flat.copy(), off.copy(), out_off.copy()
    out = np.full(int(out_off[n]) + 16, 0xCD, np.uint8)
    st2 = np.full(n, 0xEE, np.uint8)
    assert L.gsv_modexp_batch(ctx.handle, _ptr(flat), _ptr(off), n, _ptr(out), _ptr(out_off), _ptr(st2)) == 0
    assert (flat == flat0).all() and (off == off0).all() and (out_off == out_off0).all()  # inputs untouched
    assert (out[int(out_off[n]):] == 0xCD).all()
    assert list(st2) == [s for s, _ in want]
    bad = [labels[i] for i in range(n) if out[int(out_off[i]):int(out_off[i + 1])].tobytes() != want[i][1]]
    assert not bad, (len(bad), bad[:10])
    # and the Python form
    outs, st3 = ctx.modexp_batch(inputs)
    assert outs == [o for _, o in want] and list(st3) == [s for s, _ in want]


# ---------------------------------------------------------------- (c) lanes of one wave on different paths
def test_mixed_waves_of_one_class(ctx):
    items = C.mixed_wave()
    assert len(items) == 193
    want = [M.run(b) for b in items]
    mods = [M.operands(b)[2] for b in items]
    assert any(m == 0 for m in mods) and any(m == 1 for m in mods) and any(m > 1 and m & (m - 1) == 0 for m in mods)
    assert any(m % 2 for m in mods) and any(m and m % 2 == 0 and m & (m - 1) for m in mods)
    assert {M.operands(b)[1].bit_length() for b in items} >= {0, 1, 128, 256}
    outs, st = ctx.modexp_batch(items)
    assert (st == 0).all() and outs == want
    for i in (0, 63, 192):  # alone, each gives the same bytes
        o1, s1 = ctx.modexp_batch([items[i]])
        assert s1[0] == 0 and o1[0] == want[i], i


# ---------------------------------------------------------------- (d) the device-resident form
_rows = C.rows  # n rows base || exp || mod of one shape, the kinds of modulus, base and exponent in turn


def _model_rows(rows, bl, el, ml):
    return C.model_rows(M, rows, bl, el, ml)


@pytest.mark.parametrize("shape", [(32, 32, 32), (256, 3, 256), (1, 0, 1), (5, 2, 3), (33, 1, 32), (1024, 2, 1024)])
def test_device_form(ctx, shape):
    import torch
    import gsv
    bl, el, ml = shape
    n = 70 if ml > 256 else 130
    rng = random.Random(hash(shape) & 0xFFFF)
    row = bl + el + ml
    sets = [_rows(rng, n, bl, el, ml) for _ in range(2)]
    want = [_model_rows(r, bl, el, ml) for r in sets]
    dev = torch.device("cuda", ctx.device)
    G = 256  # guard bytes
    work_bytes = gsv.modexp_work_bytes(n, bl, el, ml)
    assert (work_bytes == 0) == (ml <= 32)
    ins, outs, works = [], [], []
    for r in sets:
        big = torch.zeros(n * row + 7, dtype=torch.uint8, device=dev)
        view = big[3:3 + n * row]  # an odd byte offset into a larger tensor
        view.copy_(torch.frombuffer(bytearray(b"".join(r)), dtype=torch.uint8))
        assert view.data_ptr() % 2 == 1
        ins.append(view.view(n, row))
        o = torch.full((G + n * ml + G,), 0x5A, dtype=torch.uint8, device=dev)
        outs.append(o)
        w = torch.full((G + work_bytes + G,), 0x5A, dtype=torch.uint8, device=dev)
        works.append(w)
    torch.cuda.synchronize()
    (stream,) = ctx.pipeline_streams(1)
    try:
        # two calls on the stream, nothing waited for in between: the call only enqueues
        for k in range(2):
            ctx.modexp_batch_dev(ins[k], bl, el, ml, outs[k][G:G + n * ml].view(n, ml),
                                 works[k][G:G + work_bytes] if work_bytes else None, stream=stream)
        stream.synchronize()
    finally:
        ctx.destroy_streams([stream])
    for k in range(2):
        o = outs[k].cpu().numpy()
        assert (o[:G] == 0x5A).all() and (o[G + n * ml:] == 0x5A).all(), "guard bytes around d_out"
        got = o[G:G + n * ml].tobytes()
        bad = [i for i in range(n) if got[i * ml:(i + 1) * ml] != want[k][i * ml:(i + 1) * ml]]
        assert not bad, (k, bad[:10])
        w = works[k].cpu().numpy()
        assert (w[:G] == 0x5A).all() and (w[G + work_bytes:] == 0x5A).all(), "guard bytes around d_work"
        assert (ins[k].cpu().numpy().tobytes() == b"".join(sets[k])), "d_in untouched"


# ---------------------------------------------------------------- the timing id: one launch per class
def test_kernel_time_counts_one_launch_per_class(ctx, vectors):
    from gsv import _lib
    ctx.set_timing(True)
    try:
        ctx.reset_timing()
        ctx.modexp_batch([inp for _, inp, _ in vectors])  # moduli of 32, 64, 128, 256, 512 and 1024 bytes
        ms, launches = ctx.kernel_time(_lib.K_MODEXP)
        assert launches == 6 and ms > 0
        ctx.modexp_batch([b"", C.word(1025) * 3])  # nothing reaches the device
        assert ctx.kernel_time(_lib.K_MODEXP)[1] == 6
        assert ctx.kernel_time(_lib.K_TX_SEAL)[1] == 0
    finally:
        ctx.set_timing(False)
        ctx.reset_timing()


# ---------------------------------------------------------------- (e) nothing to do
def test_empty_calls_write_nothing(ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    out = torch.full((64,), 0x5A, dtype=torch.uint8, device=dev)
    inp = torch.zeros((0, 96), dtype=torch.uint8, device=dev)
    ctx.modexp_batch_dev(inp, 32, 32, 32, out[:0].view(0, 32))
    inp = torch.full((2, 8), 3, dtype=torch.uint8, device=dev)
    ctx.modexp_batch_dev(inp, 4, 4, 0, out[:0].view(2, 0))
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A).all()
    outs, st = ctx.modexp_batch([])
    assert outs == [] and len(st) == 0
    # items without device work only: empty outputs, statuses written
    outs, st = ctx.modexp_batch([b"", C.word(3) + C.word(1) + C.word(0) + b"abcd", C.word(1025) * 3])
    assert outs == [b"", b"", b""] and list(st) == [0, 0, 15]
