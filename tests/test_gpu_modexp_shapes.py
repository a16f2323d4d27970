"""k_modexp<L> at the lengths the other modexp tests never hand it (tests/modexp_corpus.py dev_shapes, rows,
two_trip_rows), every output against the model (tests/modexp_model.py):

  test_ragged_device_form   every class at modulus lengths of every residue mod 4 on both sides of the class,
                            bases of 0 and 1 bytes, one byte either side of the modulus, with a top piece of
                            one byte and of one byte short, exponent fields of 0 and of 1024 bytes
  test_second_trip          a launch at the cap of 2,048 waves, where the lanes of waves 0 and 1 take a second
                            item on the slots (and the LDS column) their first left behind, and wave 1 leaves
                            the loop with six lanes still in it
  test_host_form_sees_item_lengths
                            one host-form call per class, so the group's widths are the items' own lengths
"""
import functools
import random

import numpy as np
import pytest

import modexp_corpus as C
import modexp_model as M

pytestmark = pytest.mark.gpu

N = 130  # two full waves and a tail of two lanes
G = 256  # guard bytes either side of d_out and d_work


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(rows, the model's outputs) of one launch of test_ragged_device_form"""
    bl, el, ml = shape
    rws = C.rows(random.Random(bl * 1000003 + el * 1009 + ml), N, bl, el, ml)
    return rws, C.model_rows(M, rws, bl, el, ml)


class _Launch:
    """the buffers of one device-form call: the input at an odd byte offset inside a larger tensor, d_out and
    d_work filled with 0x5A between guards, the work buffer of exactly the size gsv.modexp_work_bytes gives"""

    def __init__(self, ctx, data, n, bl, el, ml):
        import torch
        import gsv
        dev = torch.device("cuda", ctx.device)
        self.n, self.bl, self.el, self.ml, self.data = n, bl, el, ml, data
        row = bl + el + ml
        big = torch.zeros(n * row + 7, dtype=torch.uint8, device=dev)
        view = big[3:3 + n * row]
        view.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
        assert view.data_ptr() % 2 == 1
        self.inp = view.view(n, row)
        self.work_bytes = gsv.modexp_work_bytes(n, bl, el, ml)
        self.out = torch.full((G + n * ml + G,), 0x5A, dtype=torch.uint8, device=dev)
        self.work = torch.full((G + self.work_bytes + G,), 0x5A, dtype=torch.uint8, device=dev)

    def enqueue(self, ctx, stream):
        ctx.modexp_batch_dev(self.inp, self.bl, self.el, self.ml, self.out[G:G + self.n * self.ml].view(self.n, self.ml),
                             self.work[G:G + self.work_bytes] if self.work_bytes else None, stream=stream)

    def result(self):
        """the n * ml output bytes, once the guards and the input are seen untouched"""
        o = self.out.cpu().numpy()
        shape = (self.bl, self.el, self.ml)
        assert (o[:G] == 0x5A).all() and (o[G + self.n * self.ml:] == 0x5A).all(), ("guard bytes around d_out", shape)
        lo, hi = self.work[:G].cpu().numpy(), self.work[G + self.work_bytes:].cpu().numpy()
        assert (lo == 0x5A).all() and (hi == 0x5A).all(), ("guard bytes around d_work", shape)
        assert self.inp.cpu().numpy().tobytes() == self.data, ("d_in untouched", shape)
        return o[G:G + self.n * self.ml]


def _run(ctx, launches):
    """every launch on one stream of the context's, nothing waited for in between"""
    import torch
    torch.cuda.synchronize()
    (stream,) = ctx.pipeline_streams(1)
    try:
        for l in launches:
            l.enqueue(ctx, stream)
        stream.synchronize()
    finally:
        ctx.destroy_streams([stream])


# ---------------------------------------------------------------- (a) ragged lengths in every class
@pytest.mark.parametrize("cls", range(C.NCLASS))
def test_ragged_device_form(ctx, cls):
    shapes = C.dev_shapes(cls)
    launches = [_Launch(ctx, b"".join(_case(s)[0]), N, *s) for s in shapes]
    for l in launches:
        assert (l.work_bytes == 0) == (cls == 0)
    _run(ctx, launches)
    bad = []
    for s, l in zip(shapes, launches):
        ml = s[2]
        got, want = l.result().tobytes(), _case(s)[1]
        bad += [s + (i, "/".join(C.row_kinds(i))) for i in range(N) if got[i * ml:(i + 1) * ml] != want[i * ml:(i + 1) * ml]]
    assert not bad, (len(bad), bad[:12])


# ---------------------------------------------------------------- (b) a lane's second item
@pytest.mark.parametrize("L", [16, 128])
def test_second_trip(ctx, L):
    """L = 16: the accumulator in LDS and five numbers in the work buffer; L = 128: all six in the work buffer"""
    ml = {16: 37, 128: 259}[L]
    bl, el, n = ml + 1, 2, C.TWO_TRIP_N
    assert C.class_limbs(C.width_class(ml)) == L and n == 2048 * 64 + 70
    arr = C.two_trip_rows(random.Random(L), ml, bl, el)
    want = C.two_trip_want(M, arr, bl, el, ml)
    both = _Launch(ctx, arr.tobytes(), n, bl, el, ml)
    slots = 5 if L <= 64 else 6
    assert both.work_bytes == 2048 * 64 * slots * L * 4  # the cap on the waves is in force: the lanes come round
    second = arr[C.TWO_TRIP_LANES:]
    alone = _Launch(ctx, second.tobytes(), C.TWO_TRIP_SECOND, bl, el, ml)
    assert alone.work_bytes == 2 * 64 * slots * L * 4
    _run(ctx, [both, alone])
    got = both.result().reshape(n, ml)
    rows_bad = np.nonzero((got != want).any(axis=1))[0]
    assert rows_bad.size == 0, (rows_bad.size, [int(i) for i in rows_bad[:12]])
    # the second items alone, on slots no item has used: the same bytes
    assert alone.result().tobytes() == got[C.TWO_TRIP_LANES:].tobytes()


# ---------------------------------------------------------------- (c) the host form at a group's own lengths
def test_host_form_sees_item_lengths(ctx):
    """a call whose items all have one (bl, el, ml): the group is staged at exactly these widths, which is the
    only way the host form hands the kernel a modulus width that is no class width"""
    bad = []
    for cls in range(C.NCLASS):
        ml = C.class_edges(cls)[0] + 1
        bl, el = ml - 1, 3
        hdr = C.word(bl) + C.word(el) + C.word(ml)
        items = [hdr + r for r in C.rows(random.Random(cls), N, bl, el, ml)]
        outs, st = ctx.modexp_batch(items)
        assert (st == 0).all()
        bad += [(bl, el, ml, i, "/".join(C.row_kinds(i))) for i in range(N) if outs[i] != M.run(items[i])]
    assert not bad, (len(bad), bad[:12])
