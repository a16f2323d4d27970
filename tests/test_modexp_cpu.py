"""CPU side of the batched modexp precompile: the model tests/modexp_model.py against the reference's own
vectors (tests/golden/modexp_vectors.json), the gas restatement, the declared / exported / bound symbols,
gsv_modexp_output_layout against the model over tests/modexp_corpus.py, the argument checks of the C ABI that
need no GPU, and the device arithmetic (csrc/modexp_dev.cuh) with the host plan (csrc/modexp_plan.h) as a
stand-alone program under ASan + UBSan over the vectors and the corpus."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import modexp_corpus as C
import modexp_model as M
from conftest import ROOT, golden


@pytest.fixture(scope="module")
def vectors():
    return [(v["name"], bytes.fromhex(v["input"]), bytes.fromhex(v["expected"]))
            for v in golden("modexp_vectors.json")["vectors"]]


@pytest.fixture(scope="module")
def corpus():
    items = C.items()
    return items, [M.run_capped(b) for _, b in items]


# ---------------------------------------------------------------- the model
def test_model_reproduces_the_reference_vectors(vectors):
    assert len(vectors) == 17
    assert [n for n, _, _ in vectors[:2]] == ["eip_example1", "eip_example2"]
    assert {len(e) for _, _, e in vectors} == {32, 64, 128, 256, 512, 1024}
    for name, inp, exp in vectors:
        assert M.run(inp) == exp, name
        assert M.status(inp) == M.ST_OK


def test_gas_of_the_two_eip_examples(vectors):
    """contracts.go:167-224 by hand.  Example 1: baseLen 1, expLen 32, modLen 32; the body (65 bytes) is longer
    than baseLen and expLen <= 32, so expHead = the 32 exponent bytes ff..fe fffffc2e: BitLen 256, msb 255;
    expLen <= 32 adds nothing, adjExpLen = 255.  max(modLen, baseLen) = 32 <= 64: 32 * 32 = 1024.
    1024 * max(255, 1) / 20 = 261120 / 20 = 13056.  Example 2: baseLen 0, the same exponent and modulus: the body
    (64 bytes) is longer than 0, expHead and adjExpLen are the same, max(32, 0) = 32: 13056 again.  (EIP-198
    states 13056 for both.)"""
    from gsv import vm
    for name, inp, _ in vectors[:2]:
        assert M.required_gas(inp) == 13056, name
        assert vm.BigModExp().RequiredGas(inp) == 13056, name
    # the other arms of the formula, and the mirror against the model over the corpus' headers
    # the middle arm: max(65, 100) = 100 -> 100^2 / 4 + 96 * 100 - 3072 = 9028; expLen 40 > 32: 8 * 8 = 64, the
    # head 01 00..00 (32 bytes) has BitLen 249, msb 248: adjExpLen 312; 9028 * 312 / 20 = 140836
    two = C.encode(b"\x02" * 100, b"\x01" + bytes(39), b"\x03" * 65)
    assert M.required_gas(two) == 140836
    for _, inp in C.encodings(__import__("random").Random(1)):
        assert vm.BigModExp().RequiredGas(inp) == M.required_gas(inp)
    assert M.required_gas(C.word(2 ** 200) * 3) == 2 ** 64 - 1


def test_corpus_covers_the_axes(corpus):
    items, exp = corpus
    assert 2000 <= len(items) <= 5000
    lens = [M.lengths(b) for _, b in items]
    assert {l[2] for l in lens} >= set(C.MOD_LENS) and {l[1] for l in lens} >= set(C.EXP_LENS)
    for ml in C.MOD_LENS:
        assert {l[0] for l in lens if l[2] == ml} >= set(C.base_lens(ml)), ml
    labels = " ".join(l for l, _ in items)
    for k in C.MOD_KINDS + C.BASE_KINDS + C.EXP_KINDS:
        assert k in labels, k
    assert {st for st, _ in exp} == {M.ST_OK, M.ST_TOO_LONG}
    assert all(out == b"" for st, out in exp if st == M.ST_TOO_LONG)
    ops = [M.operands(b) for (_, b), (st, _) in zip(items, exp) if st == M.ST_OK]
    assert any(m and m % 2 == 0 and m & (m - 1) for _, _, m in ops)       # even, not a power of two
    assert any(m > 1 and m & (m - 1) == 0 for _, _, m in ops)             # a power of two
    assert any(b > m > 0 for b, _, m in ops) and any(e == 0 and b == 0 and m > 1 for b, e, m in ops)
    # the 512- and 1024-byte classes keep to 16-bit exponents
    assert all(e < 2 ** 16 + 2 for (b, e, m), l in zip(ops, [l for l, (st, _) in zip(lens, exp) if st == 0])
               if l[2] >= C.SMALL_EXP_FROM)


# ---------------------------------------------------------------- symbols and constants
def test_symbols_are_declared_exported_and_bound():
    from gsv import _lib
    L = _lib.load()
    txt = open(os.path.join(ROOT, "include", "gsv.h")).read()
    bound = {s[0] for s in _lib.SIGNATURES}
    for name in ("gsv_modexp_output_layout", "gsv_modexp_batch", "gsv_modexp_work_bytes", "gsv_modexp_batch_dev"):
        assert re.search(r"\b%s\(" % name, txt), name
        assert name in bound and getattr(L, name, None) is not None, name
    assert int(re.search(r"#define GSV_ST_MODEXP_TOO_LONG (\d+)", txt).group(1)) == _lib.ST_MODEXP_TOO_LONG == 15
    assert M.ST_TOO_LONG == _lib.ST_MODEXP_TOO_LONG
    assert int(re.search(r"#define GSV_MODEXP_MAX_LEN (\d+)", txt).group(1)) == _lib.MODEXP_MAX_LEN == M.MAX_LEN
    assert int(re.search(r"#define GSV_K_MODEXP (\d+)", txt).group(1)) == _lib.K_MODEXP == 15
    assert int(re.search(r"#define GSV_K_BOUND (\d+)", txt).group(1)) == _lib.K_MODEXP + 1
    assert int(re.search(r"#define GSV_K_LIMIT (\d+)", txt).group(1)) == 15
    assert _lib.ST_MODEXP_TOO_LONG in _lib.STATUS_STRINGS
    from gsv import vm
    assert vm.MAX_LEN == M.MAX_LEN and issubclass(vm.ErrModexpTooLong, ValueError)


def test_work_bytes():
    import gsv
    W = gsv.modexp_work_bytes
    assert W(0, 32, 32, 32) == 0 and W(1000, 32, 32, 0) == 0
    assert W(1 << 20, 1024, 1024, 32) == 0 and W(5, 1, 1, 1) == 0  # the 32-byte class keeps to registers
    for ml, limbs in ((33, 16), (64, 16), (65, 32), (128, 32), (129, 64), (256, 64), (257, 128), (512, 128),
                      (513, 256), (1024, 256)):
        slots = 5 if limbs <= 64 else 6  # up to 64 limbs the products' accumulator is in LDS
        assert W(1, 0, 0, ml) == W(64, 7, 9, ml) == 64 * slots * limbs * 4, ml
        assert W(65, 0, 0, ml) == 2 * 64 * slots * limbs * 4
        assert W(1 << 20, 0, 0, ml) == W(1 << 24, 0, 0, ml) == 2048 * 64 * slots * limbs * 4  # the launch is bounded
    assert W(1, 0, 0, 1025) == 0


# ---------------------------------------------------------------- the layout call
def test_output_layout_matches_the_model(corpus, vectors):
    import gsv
    items, exp = corpus
    inputs = [b for _, b in items] + [inp for _, inp, _ in vectors]
    want = exp + [(M.ST_OK, e) for _, _, e in vectors]
    out_off, st = gsv.modexp_output_layout(inputs)
    assert out_off[0] == 0
    assert list(np.diff(out_off.astype(np.int64))) == [len(o) for _, o in want]
    assert list(st) == [s for s, _ in want]
    o0, s0 = gsv.modexp_output_layout([])
    assert list(o0) == [0] and len(s0) == 0


# ---------------------------------------------------------------- argument errors, no GPU
def test_arguments_are_checked_without_a_device():
    from gsv import _lib
    L = _lib.load()
    EA = _lib.E_INVALID_ARG
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    inp = C.encode(b"\x03", b"\x02", b"\x07")
    data = ctypes.create_string_buffer(inp, len(inp))
    pin = ctypes.cast(data, ctypes.c_void_p)
    off = (ctypes.c_uint64 * 2)(0, len(inp))
    po = ctypes.cast(off, ctypes.c_void_p)
    down = (ctypes.c_uint64 * 2)(8, 0)
    pdown = ctypes.cast(down, ctypes.c_void_p)
    oo = (ctypes.c_uint64 * 2)(0, 0)
    poo = ctypes.cast(oo, ctypes.c_void_p)
    st = (ctypes.c_uint8 * 1)(77)
    pst = ctypes.cast(st, ctypes.c_void_p)

    lay = L.gsv_modexp_output_layout
    assert lay(pin, po, 1, poo, pst) == 0 and list(oo) == [0, 1] and st[0] == 0
    assert lay(pin, po, 1, None, pst) == EA and lay(pin, None, 1, poo, pst) == EA and lay(pin, po, 1, poo, None) == EA
    assert lay(None, po, 1, poo, pst) == EA and lay(pin, pdown, 1, poo, pst) == EA
    assert lay(None, None, 0, poo, None) == 0 and lay(None, None, 0, None, None) == EA

    def host(ctx=p, i=pin, o=po, n=1, out=p, ooff=poo, s=pst):
        return L.gsv_modexp_batch(ctx, i, o, n, out, ooff, s)

    assert host(ctx=None) == EA and host(ctx=None, n=0) == EA
    for name in ("i", "o", "out", "ooff", "s"):
        assert host(**{name: None}) == EA, name
    assert host(o=pdown) == EA and host(n=1 << 32) == EA
    for wrong in ((0, 0), (0, 2), (1, 2), (1, 1)):  # not the layout call's table
        w = (ctypes.c_uint64 * 2)(*wrong)
        assert host(ooff=ctypes.cast(w, ctypes.c_void_p)) == EA, wrong
    assert host(n=0, i=None, o=None, out=None, ooff=None, s=None) == 0

    def dev(ctx=p, i=p, n=1, bl=32, el=32, ml=32, out=p, work=p):
        return L.gsv_modexp_batch_dev(ctx, i, n, bl, el, ml, out, work, None)

    assert dev(ctx=None) == EA and dev(ctx=None, n=0) == EA
    for name in ("bl", "el", "ml"):
        assert dev(**{name: 1025}) == EA and dev(**{name: 1025}, n=0) == EA, name
    assert dev(i=None) == EA and dev(out=None) == EA and dev(n=1 << 32) == EA
    assert dev(ml=33, work=None) == EA and dev(ml=1024, work=None) == EA
    assert dev(ml=33, work=ctypes.c_void_p(p.value + 2)) == EA
    # nothing to do: success, nothing touched (the context is not a context)
    assert dev(n=0, i=None, out=None, work=None) == 0 and dev(ml=0, i=None, out=None, work=None) == 0


def test_python_mirror_checks_before_any_call():
    import gsv
    c = gsv.Context.__new__(gsv.Context)
    c._h, c.device, c._streams = None, 0, []
    outs, st = c.modexp_batch([])
    assert outs == [] and len(st) == 0

    class T:  # stands in for a tensor: the shape checks come first
        def __init__(self, n, row):
            self.shape = (n, row)
        def is_contiguous(self):
            return True
        def numel(self):
            return self.shape[0] * self.shape[1]
    with pytest.raises(ValueError):
        c.modexp_batch_dev(T(2, 96), 32, 32, 1025, T(2, 32))
    with pytest.raises(ValueError):
        c.modexp_batch_dev(T(2, 95), 32, 32, 32, T(2, 32))
    with pytest.raises(ValueError):
        c.modexp_batch_dev(T(2, 32 + 32 + 64), 32, 32, 64, T(2, 64), work_t=None)


# ---------------------------------------------------------------- the shapes of the device form
def test_dev_shapes_cover_every_class():
    shapes = C.dev_shapes()
    assert len(shapes) == len(set(shapes)) and shapes == [s for c in range(C.NCLASS) for s in C.dev_shapes(c)]
    for c in range(C.NCLASS):
        L = C.class_limbs(c)
        lo, hi = C.class_edges(c)
        assert (lo, hi) == ((1 if c == 0 else 2 * L + 1), 4 * L)
        own = C.dev_shapes(c)
        assert all(lo <= ml <= hi and C.width_class(ml) == c and bl <= 1024 and el <= 1024 for bl, el, ml in own)
        mls = {ml for _, _, ml in own}
        full = {lo, lo + 1, lo + 2, lo + 3, hi - 3, hi - 2, hi - 1, hi}
        assert mls == (full if c not in C.THIN_CLASSES else {lo, hi - 1})
        assert lo % 4 == 1 and (hi - 1) % 4 == 3 and {lo, hi - 1} <= mls  # the floor of any thinning
        assert set(C.THIN_CLASSES) <= {4, 5}
        # every kind of base length at a modulus that is no multiple of 4, under an exponent that does work
        ragged = {(bl, ml) for bl, el, ml in own if ml % 4 and 0 < el < C.WIDE_EXP_FIELD}
        for kind in C.BASE_LEN_KINDS:
            assert any(bl == C.base_len(kind, ml) for bl, ml in ragged), (c, kind)
        if 8 * L - 1 <= 1024:
            # a top piece of one byte, and one that is one byte short of full
            assert any(bl == 4 * L + 1 for bl, _ in ragged) and any(bl == 8 * L - 1 for bl, _ in ragged)
        assert any(0 < bl < ml for bl, ml in ragged) and any(bl == 0 for bl, _ in ragged)
        want_el = {0, 1, 2} if c >= 4 else {0, 1, 3, 33}
        assert {el for _, el, _ in own} == want_el | {1024}
        assert sum(el == 1024 for _, el, _ in own) == 1 and (0, 0, lo) in own
    # rows: every kind of modulus among 12 neighbouring lanes, every (modulus, base) and (base, exponent) pair
    # in a launch of 130; a 1024-byte exponent field holds 16 bits at the most
    kinds = [C.row_kinds(i) for i in range(130)]
    assert {k[0] for k in kinds[:12]} == set(C.MOD_KINDS) == {k[0] for k in kinds[118:]}
    assert {(k[0], k[1]) for k in kinds} == {(m, b) for m in C.MOD_KINDS for b in C.BASE_KINDS}
    assert {(k[1], k[2]) for k in kinds} == {(b, e) for b in C.BASE_KINDS for e in C.EXP_KINDS}
    rng = __import__("random").Random(3)
    for bl, el, ml in ((40, 1024, 39), (5, 3, 3), (0, 0, 1), (1024, 2, 1021)):
        rws = C.rows(rng, 130, bl, el, ml)
        assert len(rws) == 130 and all(len(r) == bl + el + ml for r in rws)
        exps = [int.from_bytes(r[bl:bl + el], "big") for r in rws]
        if el == 1024:
            assert max(exps) == 0xFFFF and min(exps) == 0
        mods = [int.from_bytes(r[bl + el:], "big") for r in rws]
        assert mods[4] == 0 and mods[3] == 1 and mods[0] % 2 == 1


def _path(m):
    """what an item's modulus makes the kernel do: "zero", or (k > 0, q == 1) for m = 2^k q"""
    if m == 0:
        return "zero"
    k = (m & -m).bit_length() - 1
    return (k > 0, m >> k == 1)


@pytest.fixture(scope="module")
def two_trips():
    """[(L, bl, el, ml, rows, the model's outputs)] of tests/test_gpu_modexp_shapes.py test_second_trip"""
    out = []
    for L, ml in ((16, 37), (128, 259)):
        bl, el = ml + 1, 2
        arr = C.two_trip_rows(__import__("random").Random(L), ml, bl, el)
        out.append((L, bl, el, ml, arr, C.two_trip_want(M, arr, bl, el, ml)))
    return out


def test_two_trip_rows(two_trips):
    n, lanes = 2048 * 64 + 70, 2048 * 64
    assert (C.TWO_TRIP_N, C.TWO_TRIP_LANES, C.MAX_WAVES) == (n, lanes, 2048)
    txt = open(os.path.join(ROOT, "geth-sharding_amd", "csrc", "modexp_plan.h")).read()
    assert int(re.search(r"MAX_WAVES = (\d+);", txt).group(1)) == C.MAX_WAVES
    real = C.two_trip_real()
    assert real == list(range(128)) + list(range(lanes, lanes + 70))
    for L, bl, el, ml, arr, want in two_trips:
        assert arr.shape == (n, bl + el + ml) and arr.dtype == np.uint8 and want.shape == (n, ml)
        assert C.class_limbs(C.width_class(ml)) == L
        exp = lambda i: int.from_bytes(arr[i, bl:bl + el].tobytes(), "big")
        mod = lambda i: int.from_bytes(arr[i, bl + el:].tobytes(), "big")
        assert all(exp(i) > 0 for i in real)
        # every other row is the one idle row: an odd modulus under a zero exponent, answered with 1
        idle = np.ones(n, bool)
        idle[real] = False
        assert (arr[idle] == arr[128]).all() and exp(128) == 0 and mod(128) % 2 == 1 and mod(128) > 1
        assert (want[idle] == want[128]).all() and int.from_bytes(want[128].tobytes(), "big") == 1
        for i in real:
            assert want[i].tobytes() == M.run(C.word(bl) + C.word(el) + C.word(ml) + arr[i].tobytes())
        # a lane's two items differ in path
        pairs = [(_path(mod(j)), _path(mod(lanes + j))) for j in range(70)]
        assert sum(a != b for a, b in pairs) >= 40
        odd = (False, False)
        assert ("zero", odd) in pairs and (odd, "zero") in pairs
        wide = lambda i: mod(i) and (mod(i) & -mod(i)).bit_length() - 1 >= 32 and _path(mod(i)) == (True, False)
        plain = lambda i: mod(i) and (mod(i) % 2 == 1 or _path(mod(i))[1])  # odd, or a power of two
        assert any(wide(j) and plain(lanes + j) for j in range(70))
        assert any(plain(j) and wide(lanes + j) for j in range(70))
        assert {_path(mod(j)) for j in range(12)} == {"zero", (False, False), (False, True), (True, False), (True, True)}


# ---------------------------------------------------------------- the arithmetic, as host code under sanitizers
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """tests/native/modexp_host_main.cpp with ASan + UBSan (a plain build where the compiler links neither)"""
    src = os.path.join(ROOT, "tests", "native", "modexp_host_main.cpp")
    exe = tmp_path_factory.mktemp("modexp_host") / "modexp_host_main"
    base = ["g++", "-O2", "-g", "-std=c++17", "-Wall", "-o", str(exe), src]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    return str(exe)


def _write_items(path, pairs):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(pairs)))
        for inp, out in pairs:
            f.write(struct.pack("<II", len(inp), len(out)) + inp + out)


def test_device_arithmetic_as_host_code_under_sanitizers(tmp_path, host_exe, corpus, vectors):
    """csrc/modexp_dev.cuh and csrc/modexp_plan.h as a stand-alone program with ASan + UBSan (a plain build
    where the compiler links neither), run as a child process over the vectors, the corpus and the mixed wave of
    the GPU test, through every width class: tests/native/modexp_host_main.cpp"""
    items, exp = corpus
    pairs = [(inp, e) for _, inp, e in vectors] + [(b, out) for (_, b), (_, out) in zip(items, exp)]
    pairs += [(b, M.run(b)) for b in C.mixed_wave()]
    data = tmp_path / "modexp_items.bin"
    _write_items(data, pairs)
    r = subprocess.run([host_exe, str(data)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_interleaved_region_and_dirty_slots_under_sanitizers(tmp_path, host_exe, two_trips):
    """The instantiation the kernel runs, modexp_item<L, 64, false> on the columns of a wave's region of
    exactly work_bytes, for every class: the rows of dev_shapes() (twelve rows a shape, five in the two widest
    classes, the kinds moving on from shape to shape), then the twice-used lanes of two_trip_rows(), a lane's
    first item and then its second.  The program runs the items of a class one after the other in one column
    that is never cleared, and each of them again on slots of 0x00, of 0xFF and of a pattern."""
    rng = __import__("random").Random(64)
    pairs = []
    for k, (bl, el, ml) in enumerate(C.dev_shapes()):
        per = 5 if ml >= C.SMALL_EXP_FROM else 12
        hdr = C.word(bl) + C.word(el) + C.word(ml)
        pairs += [(hdr + r, M.run(hdr + r)) for r in C.rows(rng, per, bl, el, ml, start=k * per)]
    for L, bl, el, ml, arr, want in two_trips:
        hdr = C.word(bl) + C.word(el) + C.word(ml)
        for j in range(C.TWO_TRIP_SECOND):
            for i in (j, C.TWO_TRIP_LANES + j):
                pairs.append((hdr + arr[i].tobytes(), want[i].tobytes()))
    assert {C.width_class(M.lengths(inp)[2]) for inp, _ in pairs} == set(range(C.NCLASS))
    data = tmp_path / "modexp_region.bin"
    _write_items(data, pairs)
    r = subprocess.run([host_exe, "--region", str(data)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    assert "%d runs" % (4 * len(pairs)) in r.stderr
