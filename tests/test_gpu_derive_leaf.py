"""GPU: k_derive_leaf / keccak_hdr_value (csrc/chunk_root.hip) at every hashed length T = H + L around the
inline threshold and the Keccak rate blocks, on both of its load paths and at the four byte alignments of the
values, through gsv_derive_sha_batch_dev against oracle.derive_sha.  The lengths and the two leaf classes are
tests/derive_leaf_model.py's, pinned to the oracle by tests/test_derive_leaf_cpu.py.

The kernel reads a value in whole 16-byte groups when no lane of the wave has a value within 32 bytes of the
batch's first or last byte (`edge`, the ballot before keccak_hdr_value in k_derive_leaf), else dword by dword.
Leaves are launched per list length N, and wg_bucket_order (csrc/keccak_dev.cuh) puts a launch of at most 64
leaves into wave 0, so a test chooses the path by what it puts into one call; each run asserts from the
offsets that it got the path it is named after."""
from collections import namedtuple

import numpy as np
import pytest

import derive_leaf_model as M

pytestmark = pytest.mark.gpu

GUARD = 64  # bytes of 0xEE before and behind the values
Entry = namedtuple("Entry", "N tag values root")  # one list: N values of one length; tag = its L (or "1<80", "1>=80")


def _entries(oracle, rng, Ns, lens):
    out = []
    for N in Ns:
        for L in lens:
            if L == 1:  # a byte below 0x80 is its own RLP and never goes through keccak_hdr_value; one from 0x80 up does
                sets = [("1<80", rng.integers(0, 0x80, (N, 1), dtype=np.uint8)),
                        ("1>=80", rng.integers(0x80, 0x100, (N, 1), dtype=np.uint8))]
            else:
                sets = [(L, rng.integers(0, 256, (N, L), dtype=np.uint8))]
            for tag, a in sets:
                values = [row.tobytes() for row in a]
                out.append(Entry(N, tag, values, oracle.derive_sha(values)))
    return out


def _guard(oracle, rng, N):
    return _entries(oracle, rng, [N], [64])[0]


@pytest.fixture(scope="module")
def sweep(oracle):
    """every (N, L) list of the short sweep with its root, and the three-item lists that bracket a batch"""
    rng = np.random.default_rng(136)
    ent = _entries(oracle, rng, (1, 2, 17, 130), M.SWEEP_L)
    assert len(ent) == 4 * 422 and sum(e.N for e in ent) == 63300
    return ent, _guard(oracle, rng, 3)


@pytest.fixture(scope="module")
def long_sweep(oracle):
    rng = np.random.default_rng(65536)
    return _entries(oracle, rng, (1, 3), M.LONG_L), _guard(oracle, rng, 2)


def _reg_hashed(N, v):
    """does k_derive_leaf hash this leaf through keccak_hdr_value?"""
    if len(v) == 1 and v[0] < 0x80:
        return False
    return N == 1 or M.hashed_len(M.CLASS_OF_N[N], len(v)) >= 32


def _run(ctx, entries, shift, path):
    """one gsv_derive_sha_batch_dev call over `entries` with the values `shift` bytes into a 16-byte aligned
    tensor; returns the (N, tag) of every list whose root differs"""
    import torch
    items = [(e.N, v) for e in entries for v in e.values]
    lens = np.fromiter((len(v) for _, v in items), np.uint64, len(items))
    voff = np.zeros(len(items) + 1, np.uint64)
    np.cumsum(lens, out=voff[1:])
    list_off = np.cumsum([0] + [e.N for e in entries]).astype(np.uint64)
    vend = int(voff[-1])
    at_edge = (voff[:-1] < 32) | (voff[1:] + 32 > vend)
    hashed = np.fromiter((_reg_hashed(N, v) for N, v in items), bool, len(items))
    if path == "interior":  # the bracketing lists have an N of their own: their launch is not a swept one
        swept = np.ones(len(items), bool)
        swept[:entries[0].N] = swept[-entries[-1].N:] = False
        assert entries[0].N == entries[-1].N and all(e.N != entries[0].N for e in entries[1:-1])
        assert not (at_edge & swept).any()
    else:  # one launch, one wave, and a hashed leaf at the batch's edge in it
        assert len({e.N for e in entries}) == 1 and len(items) <= 64
        assert not hashed.any() or (hashed & at_edge).any()
    flat = np.frombuffer(b"".join(v for _, v in items), np.uint8)
    host = np.full(GUARD + shift + len(flat) + GUARD, 0xEE, np.uint8)
    host[GUARD + shift:GUARD + shift + len(flat)] = flat
    base = torch.from_numpy(host).cuda()
    assert base.data_ptr() % 16 == 0
    vals = base[GUARD + shift:GUARD + shift + len(flat)]
    roots = torch.zeros((len(entries), 32), dtype=torch.uint8, device="cuda")
    ctx.derive_sha_batch_dev(vals, voff, list_off, roots)
    torch.cuda.synchronize()
    assert base.cpu().numpy().tobytes() == host.tobytes(), "the input changed"
    r = roots.cpu().numpy()
    return [(e.N, e.tag) for i, e in enumerate(entries) if bytes(r[i]) != e.root]


def _run_edge(ctx, entries, shift, per_call):
    bad = []
    for k in range(0, len(entries), per_call):
        bad += _run(ctx, entries[k:k + per_call], shift, "edge")
    return bad


def _report(bad):
    assert not bad, "%d lists differ, (N, L): %s" % (len(bad), bad)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_leaf_sweep_interior_waves(ctx, sweep, shift):
    """The 16-byte-group path.  One batch of N = 1, 2, 17 and 130 values for every L in 0...420 (63,300 leaves,
    13 MB) between two lists of three 64-byte values: no swept value lies within 32 bytes of the batch's ends,
    and a leaf launch covers the lists of one N, so in every swept wave the ballot of `edge` in k_derive_leaf
    (`bool edge = voff[item] < voff[0] + 32 || voff[item + 1] + 32 > vend`) is zero and keccak_hdr_value runs
    with whole = true.  The values start `shift` bytes into a 16-byte aligned tensor: every leaf at all four
    residues of (v - H) & 3."""
    ent, guard = sweep
    _report(_run(ctx, [guard] + ent + [guard], shift, "interior"))


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_leaf_sweep_edge_waves(ctx, sweep, shift):
    """The dword path.  A call of at most 64 leaves is one wave, which holds a leaf at the batch's edge, so
    keccak_hdr_value runs with whole = false: N = 1 (64 lists a call) and N = 2 (32 lists) at every L in
    0...420, N = 17 (three lists) at the model's EDGE_L."""
    ent, _ = sweep
    bad = _run_edge(ctx, [e for e in ent if e.N == 1], shift, 64)
    bad += _run_edge(ctx, [e for e in ent if e.N == 2], shift, 32)
    edge_l = set(M.EDGE_L) | {"1<80", "1>=80"}
    e17 = [e for e in ent if e.N == 17 and e.tag in edge_l]
    assert len(e17) >= len(M.EDGE_L)
    bad += _run_edge(ctx, e17, shift, 3)
    _report(bad)


@pytest.mark.parametrize("shift", [0, 3])
def test_leaf_long_prefix_edges(ctx, long_sweep, shift):
    """Values of 65,500...65,559 bytes, N = 1 and 3: the string prefix goes from three to four bytes at 65,536
    and the list prefix at a payload of 65,536 (L = 65,530 / 65,532), so H takes 9, 10, 11 and 7, 8, 9 bytes.
    Once between two lists of two 64-byte values (the 16-byte-group path) and once in calls of at most 64
    leaves (the dword path)."""
    ent, guard = long_sweep
    bad = _run(ctx, [guard] + ent + [guard], shift, "interior")
    bad += _run_edge(ctx, [e for e in ent if e.N == 1], shift, 64)
    bad += _run_edge(ctx, [e for e in ent if e.N == 3], shift, 21)
    _report(bad)


def test_leaf_sweep_host_form(ctx, sweep):
    """gsv_derive_sha_batch (host pointers, staged by the library) over the interior batch's lists"""
    ent, guard = sweep
    ent = [guard] + ent + [guard]
    out = ctx.derive_sha_batch([e.values for e in ent])
    _report([(e.N, e.tag) for i, e in enumerate(ent) if bytes(out[i]) != e.root])
