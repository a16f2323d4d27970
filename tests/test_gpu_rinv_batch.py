"""GPU parity of recovery with r^-1 taken from the batched pass (k_rinv_batch + k_ecrecover<true>,
geth-sharding_amd/csrc/ecrecover.hip): the device-resident call with a pub65 output, which stashes the
inverses in that output, against the oracle byte for byte and against the same call without pub65
(every lane inverts its own r).  Batch sizes sit on the group, wave and block boundaries of the two
kernels; invalid r, s and recid are placed first, in the middle and last among the items one lane of the
new kernel handles (rows 64 apart) and among RINV_K consecutive items."""
import random

import numpy as np
import pytest

from test_rinv_batch import K, N

pytestmark = pytest.mark.gpu
GUARD = 0xFF
PAD = 3  # the pub65 output starts this many bytes into its allocation: no alignment to lean on
SIZES = [1, K - 1, K, K + 1, 64 * K - 1, 64 * K + 1]
BIG = 64 * K + 1


def be(v):
    return np.frombuffer(int(v).to_bytes(32, "big"), np.uint8)


# r out of range, s out of range, recid with the r + n bit / out of range
BAD = [("r", 0), ("r", N), ("r", N + 1), ("r", 2**256 - 1), ("s", 0), ("s", N),
       ("v", 2), ("v", 3), ("v", 4), ("v", 255)]


def bad_rows(n):
    """row -> kind.  Kind j sits first, in the middle and last of lane j's rows (j, j + 64, ...), of the
    RINV_K consecutive rows from RINV_K (j + 2) on, and of the batch."""
    want = []
    for j in range(len(BAD)):
        want += [(j, j), (64 * (K // 2) + j, j), (64 * (K - 1) + j, j)]
        want += [(K * (j + 2), j), (K * (j + 2) + K // 2, j), (K * (j + 2) + K - 1, j)]
    want += [(0, 0), (n // 2, 5), (n - 1, 3), (n - 2, 9)]
    rows = {}
    for row, j in want:
        if 0 <= row < n:
            rows.setdefault(row, j)
    return rows


@pytest.fixture(scope="module")
def signed(oracle):
    """BIG valid signatures from the oracle signer"""
    rng = random.Random(0x10)
    msg = np.zeros((BIG, 32), np.uint8)
    sig = np.zeros((BIG, 65), np.uint8)
    for i in range(BIG):
        m = bytes(rng.getrandbits(8) for _ in range(32))
        s = oracle.secp_sign(m, rng.randrange(1, N).to_bytes(32, "big"), rng.randrange(1, N).to_bytes(32, "big"))
        msg[i] = np.frombuffer(m, np.uint8)
        sig[i] = np.frombuffer(s, np.uint8)
    return msg, sig


@pytest.fixture(scope="module")
def cases(signed, oracle):
    """per batch size: (msg, sig, oracle pub65, oracle addr20, oracle status, rows made invalid), built once"""
    out = {}
    for n in SIZES:
        msg, sig = signed[0][:n].copy(), signed[1][:n].copy()
        rows = bad_rows(n) if n > 1 else {}
        for row, j in rows.items():
            what, v = BAD[j]
            if what == "r":
                sig[row, :32] = be(v)
            elif what == "s":
                sig[row, 32:64] = be(v)
            else:
                sig[row, 64] = v
        pub, st = oracle.ecrecover_batch(msg, sig)
        addr = np.zeros((n, 20), np.uint8)
        for i in np.nonzero(st == 0)[0]:
            addr[i] = np.frombuffer(oracle.keccak256(bytes(pub[i, 1:]))[12:], np.uint8)
        # the invalid items fail and are zeroed, every neighbour recovers
        assert all(st[r] != 0 and not pub[r].any() for r in rows)
        assert all(st[i] == 0 and pub[i, 0] == 4 for i in range(n) if i not in rows)
        if n > 1:
            assert {j for j in rows.values()} == set(range(len(BAD)))
        out[n] = (msg, sig, pub, addr, st, rows)
    return out


class Outputs:
    """pub65 at an odd offset inside a larger allocation, addr20 and status, all pre-filled with GUARD"""

    def __init__(self, dev, n, want_pub=True):
        import torch
        self.n = n
        self.raw = torch.full((PAD + n * 65 + 61,), GUARD, dtype=torch.uint8, device=dev)
        self.pub = self.raw[PAD:PAD + n * 65].view(n, 65) if want_pub else None
        self.addr = torch.full((n, 20), GUARD, dtype=torch.uint8, device=dev)
        self.st = torch.full((n,), GUARD, dtype=torch.uint8, device=dev)
        if want_pub:
            assert self.pub.data_ptr() % 4 == PAD

    def refill(self):
        self.raw.fill_(GUARD)
        self.addr.fill_(GUARD)
        self.st.fill_(GUARD)

    def check(self, case, pub=True):
        _, _, opub, oaddr, ost, _ = case
        raw = self.raw.cpu().numpy()
        st, addr = self.st.cpu().numpy(), self.addr.cpu().numpy()
        assert (st == ost).all(), np.nonzero(st != ost)[0][:10]
        assert (addr == oaddr).all(), np.nonzero((addr != oaddr).any(axis=1))[0][:10]
        n = self.n
        if pub:
            got = raw[PAD:PAD + n * 65].reshape(n, 65)
            assert (got == opub).all(), np.nonzero((got != opub).any(axis=1))[0][:10]
            assert (raw[:PAD] == GUARD).all() and (raw[PAD + n * 65:] == GUARD).all()  # nothing outside n * 65 bytes
        else:
            assert (raw == GUARD).all()


def upload(ctx, case):
    import torch
    dev = torch.device("cuda", ctx.device)
    return dev, torch.from_numpy(case[0]).to(dev), torch.from_numpy(case[1]).to(dev)


@pytest.mark.parametrize("n", SIZES)
def test_stashed_inverse_matches_oracle_and_own_inversion(ctx, cases, n):
    import torch
    case = cases[n]
    dev, d_msg, d_sig = upload(ctx, case)
    a, b = Outputs(dev, n), Outputs(dev, n, want_pub=False)
    ctx.ecrecover_batch_dev(d_msg, d_sig, a.pub, a.addr, a.st)
    ctx.ecrecover_batch_dev(d_msg, d_sig, None, b.addr, b.st)  # no pub65: no stash, k_ecrecover<false>
    torch.cuda.synchronize()
    a.check(case)
    b.check(case, pub=False)
    assert torch.equal(a.addr, b.addr) and torch.equal(a.st, b.st)


def test_host_form_matches_oracle(ctx, cases):
    msg, sig, opub, oaddr, ost, _ = cases[64 * K - 1]
    pub, addr, st = ctx.ecrecover_batch(msg, sig, want_pub=True, want_addr=True)
    assert (st == ost).all() and (pub == opub).all() and (addr == oaddr).all()


def test_two_streams_into_two_output_sets(ctx, cases):
    """the bench's shape: two batches in flight on two streams, each into its own outputs"""
    import torch
    case = cases[BIG]
    dev, d_msg, d_sig = upload(ctx, case)
    outs = [Outputs(dev, BIG), Outputs(dev, BIG)]
    torch.cuda.synchronize()
    streams = ctx.pipeline_streams(2)
    try:
        for _ in range(2):
            for o, s in zip(outs, streams):
                ctx.ecrecover_batch_dev(d_msg, d_sig, o.pub, o.addr, o.st, stream=s)
        for s in streams:
            s.synchronize()
    finally:
        ctx.destroy_streams(streams)
    single = Outputs(dev, BIG)
    ctx.ecrecover_batch_dev(d_msg, d_sig, single.pub, single.addr, single.st)
    torch.cuda.synchronize()
    single.check(case)
    for o in outs:
        o.check(case)
        assert torch.equal(o.raw, single.raw) and torch.equal(o.addr, single.addr) and torch.equal(o.st, single.st)


def test_captured_call_replays(ctx, cases):
    import torch
    n = 64 * K + 1
    case = cases[n]
    dev, d_msg, d_sig = upload(ctx, case)
    o = Outputs(dev, n)
    torch.cuda.synchronize()
    cs = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    shapes_before = ctx.prepared_shapes()
    with torch.cuda.graph(g, stream=cs):
        ctx.ecrecover_batch_dev(d_msg, d_sig, o.pub, o.addr, o.st, stream=cs)
    assert ctx.prepared_shapes() == shapes_before  # nothing allocated inside the capture
    for _ in range(2):
        o.refill()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        o.check(case)


def test_one_timed_interval_per_call(ctx, cases):
    """both launches of a call are one K_ECRECOVER interval"""
    import torch
    from gsv import _lib
    case = cases[K + 1]
    dev, d_msg, d_sig = upload(ctx, case)
    o = Outputs(dev, K + 1)
    ctx.set_timing(True)
    try:
        ctx.reset_timing()
        ctx.ecrecover_batch_dev(d_msg, d_sig, o.pub, o.addr, o.st)
        torch.cuda.synchronize()
        ms, launches = ctx.kernel_time(_lib.K_ECRECOVER)
        assert launches == 1 and ms > 0
    finally:
        ctx.set_timing(False)
        ctx.reset_timing()
    o.check(case)
