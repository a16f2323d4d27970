"""GPU parity of batched ecies.Decrypt / Encrypt (k_ecies_parse, k_ecdh, k_ecies_open / k_ecies_seal) with
the reference's own handshake packets (tests/golden/ecies_rlpx.json, from p2p/rlpx_test.go), the recorded
rows of tests/golden/ecies.json and the Python model (tests/ecies_model.py).  Every comparison is byte
for byte over every item and covers status and msg_len.  The _dev forms run on an explicit stream with
every output over-allocated and pre-filled with 0xEE: nothing outside an item's slot may change, a slot
past msg_len is zero, a failed slot is all zero, and the work area is all zero afterwards.  No test
provokes a fault: every malformed input is a defined status."""
import ctypes

import numpy as np
import pytest

import ecies_model as M
from conftest import golden

pytestmark = pytest.mark.gpu
GUARD = 0xEE
TAIL = 24  # guard bytes behind every over-allocated buffer
SHAPES = [1, 63, 64, 65, 257]
OV = M.OVERHEAD


def u8(b, width):
    return np.frombuffer(bytes(b), np.uint8).reshape(-1, width).copy()


def packed(items, base):
    """byte strings back to back from `base` on inside a guard-filled buffer: (buffer, int64 offsets)"""
    off = np.zeros(len(items) + 1, np.int64)
    off[0] = base
    np.cumsum([len(x) for x in items], out=off[1:])
    off[1:] += base
    buf = np.full(int(off[-1]) + TAIL, GUARD, np.uint8)
    flat = b"".join(items)
    buf[base:base + len(flat)] = np.frombuffer(flat, np.uint8)
    return buf, off


def tdev(ctx, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", ctx.device))


def tfull(ctx, n, dtype=None):
    import torch
    dtype = dtype or torch.uint8
    fill = GUARD if dtype == torch.uint8 else 0x6EEEEEEE
    return torch.full((n,), fill, dtype=dtype, device=torch.device("cuda", ctx.device))


class DevDecrypt:
    """one gsv_ecies_decrypt_batch_dev call's device buffers; run() enqueues it on `stream`"""

    def __init__(self, ctx, cts, keys, s2s, base=3):
        import torch
        self.ctx, self.n = ctx, len(cts)
        buf, self.off = packed(cts, base)
        self.d_ct, self.d_off, self.d_key = tdev(ctx, buf), tdev(ctx, self.off), tdev(ctx, u8(b"".join(keys), 32))
        self.d_s2 = self.d_s2off = None
        if s2s is not None:
            sbuf, soff = packed(s2s, 1)
            self.d_s2, self.d_s2off = tdev(ctx, sbuf), tdev(ctx, soff)
        self.wb = int(M_lib().gsv_ecies_work_bytes(self.n, 0))
        self.d_msg, self.d_mlen = tfull(ctx, buf.size), tfull(ctx, self.n + 1, torch.int32)
        self.d_st, self.d_work = tfull(ctx, self.n + 1), tfull(ctx, self.wb + TAIL)

    def run(self, stream):
        self.ctx.ecies_decrypt_batch_dev(self.d_ct, self.d_off, self.d_key, self.d_s2, self.d_s2off, self.d_msg,
                                         self.d_mlen, self.d_st, self.d_work, stream=stream)

    def check(self, want):
        """want: [(status, msg)].  Everything the call may and may not have written."""
        n, off = self.n, self.off
        msg, mlen = self.d_msg.cpu().numpy(), self.d_mlen.cpu().numpy()
        st, work = self.d_st.cpu().numpy(), self.d_work.cpu().numpy()
        assert list(st[:n]) == [s for s, _ in want], np.nonzero(st[:n] != np.array([s for s, _ in want]))[0][:10]
        assert list(mlen[:n]) == [len(m) for _, m in want]
        for i, (s, m) in enumerate(want):
            slot = msg[off[i]:off[i + 1]]
            assert bytes(slot[:len(m)]) == m, i
            assert not slot[len(m):].any(), i  # past msg_len: zeros; a failed slot: all zeros
        assert (msg[:off[0]] == GUARD).all() and (msg[off[n]:] == GUARD).all()
        assert st[n] == GUARD and mlen[n] == 0x6EEEEEEE
        assert not work[:self.wb].any(), "the work area holds something after the call"
        assert (work[self.wb:] == GUARD).all()


class DevEncrypt:
    def __init__(self, ctx, msgs, pubs, ephs, ivs, s2s, base=2):
        self.ctx, self.n = ctx, len(msgs)
        buf, self.off = packed(msgs, base)
        self.d_msg, self.d_off = tdev(ctx, buf), tdev(ctx, self.off)
        self.d_pub, self.d_eph = tdev(ctx, u8(b"".join(pubs), 64)), tdev(ctx, u8(b"".join(ephs), 32))
        self.d_iv = tdev(ctx, u8(b"".join(ivs), 16))
        self.d_s2 = self.d_s2off = None
        if s2s is not None:
            sbuf, soff = packed(s2s, 3)
            self.d_s2, self.d_s2off = tdev(ctx, sbuf), tdev(ctx, soff)
        self.wb = int(M_lib().gsv_ecies_work_bytes(self.n, 1))
        self.pos = [int(self.off[i]) + OV * i for i in range(self.n + 1)]  # item i at msg_off[i] + 113 i
        self.d_ct, self.d_st = tfull(ctx, self.pos[-1] + TAIL), tfull(ctx, self.n + 1)
        self.d_work = tfull(ctx, self.wb + TAIL)

    def run(self, stream):
        self.ctx.ecies_encrypt_batch_dev(self.d_msg, self.d_off, self.d_pub, self.d_eph, self.d_iv, self.d_s2,
                                         self.d_s2off, self.d_ct, self.d_st, self.d_work, stream=stream)

    def check(self, want):
        """want: [(status, ct)]"""
        n, pos = self.n, self.pos
        ct, st, work = self.d_ct.cpu().numpy(), self.d_st.cpu().numpy(), self.d_work.cpu().numpy()
        assert list(st[:n]) == [s for s, _ in want]
        for i, (s, c) in enumerate(want):
            assert bytes(ct[pos[i]:pos[i + 1]]) == c, i
        assert (ct[:pos[0]] == GUARD).all() and (ct[pos[n]:] == GUARD).all() and st[n] == GUARD
        assert not work[:self.wb].any(), "the work area holds something after the call"
        assert (work[self.wb:] == GUARD).all()


def M_lib():
    from gsv import _lib
    return _lib.load()


def on_stream(*calls):
    import torch
    torch.cuda.synchronize()
    cs = torch.cuda.Stream()
    for c in calls:
        c.run(cs)
    cs.synchronize()


@pytest.fixture(scope="module")
def rows():
    """the reference's six packets, the fixture's rows Decrypt opens, and its bad rows:
    ([(ct, key, s2)], [(status, msg)])"""
    rl, fx = golden("ecies_rlpx.json"), golden("ecies.json")
    items, want = [], []
    for p in rl["packets"]:
        raw = bytes.fromhex(p["packet"])
        s2, c = (raw[:2], raw[2:]) if p["eip8"] else (b"", raw)
        items.append((c, bytes.fromhex(rl[p["key"]]), s2))
        want.append(M.decrypt(c, items[-1][1], s2))
    assert [s for s, _ in want] == [0] * 6 and [len(m) for _, m in want] == [194, 322, 327, 97, 377, 383]
    for r in fx["good"]:
        if r["status"] == 0:
            items.append((bytes.fromhex(r["ct"]), bytes.fromhex(r["seckey"]), bytes.fromhex(r["s2"])))
            want.append((0, bytes.fromhex(r["msg"])))
    for r in fx["bad"]:
        items.append((bytes.fromhex(r["ct"]), bytes.fromhex(r["seckey"]), bytes.fromhex(r["s2"])))
        want.append((r["status"], bytes.fromhex(r["msg"])))
    return items, want


@pytest.fixture(scope="module")
def pool():
    """257 seeded items of mixed lengths, computed once (ecies_model.batch_items)"""
    items = M.batch_items(257)
    assert (len(items[2][0]), len(items[3][0])) == (0, 1000)
    assert {sum(len(x[6]) for x in items[:k]) % 4 for k in range(64)} == {0, 1, 2, 3}  # every residue of an offset
    return items


# ---------------------------------------------------------------- 1. recorded rows
def test_packets_and_fixture_rows_host_dev_and_mirrors(ctx, rows):
    from gsv import _lib, ecies
    items, want = rows
    cts, keys, s2s = [c for c, _, _ in items], [k for _, k, _ in items], [s for _, _, s in items]
    karr = u8(b"".join(keys), 32)
    msgs, st = ctx.ecies_decrypt_batch(cts, karr, s2s)
    assert list(st) == [s for s, _ in want], [(i, st[i], want[i][0]) for i in range(len(want)) if st[i] != want[i][0]]
    assert msgs == [m for _, m in want]
    d = DevDecrypt(ctx, cts, keys, s2s)
    on_stream(d)
    d.check(want)
    m2, st2 = ecies.DecryptBatch(karr, cts, s2s, ctx)
    assert m2 == msgs and (st2 == st).all()
    # the six packets and one row of each status through the one-item mirror
    errs = {_lib.ST_INVALID_MESSAGE: ecies.ErrInvalidMessage, _lib.ST_INVALID_PUBKEY: ecies.ErrInvalidPublicKey,
            _lib.ST_INVALID_CURVE: ecies.ErrInvalidCurve, _lib.ST_INVALID_KEY: ecies.ErrSharedKeyIsPointAtInfinity}
    seen = set()
    for i, ((c, k, s2), (s, m)) in enumerate(zip(items, want)):
        if i >= 6 and s in seen:
            continue
        seen.add(s)
        if s == 0:
            assert ecies.Decrypt(k, c, None, s2, ctx) == m
        else:
            with pytest.raises(errs[s]):
                ecies.Decrypt(k, c, None, s2, ctx)
    assert seen == {0, 7, 11, 12, 14}
    # no s2 table at all: the two pre-EIP-8 packets
    plain = [0, 3]
    msgs, st = ctx.ecies_decrypt_batch([cts[i] for i in plain], karr[plain], None)
    assert list(st) == [0, 0] and msgs == [want[i][1] for i in plain]
    d = DevDecrypt(ctx, [cts[i] for i in plain], [keys[i] for i in plain], None)
    on_stream(d)
    d.check([want[i] for i in plain])


def test_encrypt_fixture_rows_host_dev_and_mirrors(ctx):
    from gsv import ecies
    good = golden("ecies.json")["good"]
    f = [[bytes.fromhex(r[k]) for r in good] for k in ("msg", "pub", "eph", "iv", "s2", "ct", "seckey")]
    msgs, pubs, ephs, ivs, s2s, cts, sks = f
    want = [(r["status"], c) for r, c in zip(good, cts)]
    got, st = ctx.ecies_encrypt_batch(msgs, u8(b"".join(pubs), 64), u8(b"".join(ephs), 32), u8(b"".join(ivs), 16), s2s)
    assert list(st) == [s for s, _ in want] and got == cts
    e = DevEncrypt(ctx, msgs, pubs, ephs, ivs, s2s)
    on_stream(e)
    e.check(want)
    g2, st2 = ecies.EncryptBatch(msgs, u8(b"".join(pubs), 64), u8(b"".join(ephs), 32), u8(b"".join(ivs), 16), s2s, ctx)
    assert g2 == cts and (st2 == st).all()
    # the one-item mirror with a scripted rand: a key of 0 and one >= n are drawn again
    j = 5
    feed = [bytes(32), b"\xff" * 32, ephs[j], ivs[j]]
    assert ecies.Encrypt(lambda k: feed.pop(0), pubs[j], msgs[j], None, s2s[j], ctx) == cts[j] and not feed
    feed = [ephs[j], ivs[j]]
    assert ecies.Encrypt(lambda k: feed.pop(0), b"\x04" + pubs[j], b"", None, None, ctx) == b""
    assert ecies.Decrypt(sks[j], cts[j], None, s2s[j], ctx) == msgs[j]
    with pytest.raises(ecies.ErrInvalidCurve):
        ecies.Encrypt(lambda k: bytes([1]) * k, (M.E.GX, M.E.GY + 1), b"m", ctx=ctx)


# ---------------------------------------------------------------- 2. launch shapes
@pytest.mark.parametrize("n", SHAPES)
def test_launch_shapes(ctx, pool, n):
    it = pool[:n]
    msgs, pubs, sks, ephs, ivs, s2s, cts = (list(x) for x in zip(*it))
    want_d = [(0, m) for m in msgs]
    want_e = [(0, c) if m else (M.ST_INVALID_MESSAGE, bytes(OV)) for m, c in zip(msgs, cts)]
    d, e = DevDecrypt(ctx, cts, sks, s2s), DevEncrypt(ctx, msgs, pubs, ephs, ivs, s2s)
    on_stream(d, e)
    d.check(want_d)
    e.check(want_e)
    got, st = ctx.ecies_decrypt_batch(cts, u8(b"".join(sks), 32), s2s)
    assert not st.any() and got == msgs
    got, st = ctx.ecies_encrypt_batch(msgs, u8(b"".join(pubs), 64), u8(b"".join(ephs), 32), u8(b"".join(ivs), 16), s2s)
    assert list(st) == [s for s, _ in want_e] and got == [c for _, c in want_e]


# ---------------------------------------------------------------- 3. failures among good items
def test_every_failure_class_beside_good_items(ctx, pool):
    fx = golden("ecies.json")
    bad = [(bytes.fromhex(r["ct"]), bytes.fromhex(r["seckey"]), bytes.fromhex(r["s2"]), r["status"],
            bytes.fromhex(r["msg"])) for r in fx["bad"]]
    assert {b[3] for b in bad} == {0, 7, 11, 12, 14}
    cts, keys, s2s, want = [], [], [], []
    for j, b in enumerate(bad):  # good, bad, good, bad, ...: every bad item between two good ones
        g = pool[j]
        cts += [g[6], b[0]]
        keys += [g[2], b[1]]
        s2s += [g[5], b[2]]
        want += [(0, g[0]), (b[3], b[4])]
    d = DevDecrypt(ctx, cts, keys, s2s)
    on_stream(d)
    d.check(want)
    msgs, st = ctx.ecies_decrypt_batch(cts, u8(b"".join(keys), 32), s2s)
    assert list(st) == [s for s, _ in want] and msgs == [m for _, m in want]
    # Encrypt's three failures, each beside good items
    g = pool[:8]
    msgs, pubs, sks, ephs, ivs, s2s, cts = (list(x) for x in zip(*g))
    off = M.E.be32(M.E.GX) + M.E.be32(M.E.GY + 1)
    ephs[1], ephs[5] = bytes(32), M.E.be32(M.E.N)
    pubs[4] = off
    pubs[5] = off  # a bad key and a point off the curve: the key rule first
    want = [M.encrypt(*a) for a in zip(msgs, pubs, ephs, ivs, s2s)]
    assert [s for s, _ in want] == [0, 11, 14, 0, 12, 11, 0, 0]
    e = DevEncrypt(ctx, msgs, pubs, ephs, ivs, s2s)
    on_stream(e)
    e.check(want)


# ---------------------------------------------------------------- 4. device-resident round trip
def test_encrypt_then_decrypt_without_a_host_round_trip(ctx, pool):
    import torch
    it = [x for x in pool[:130] if x[0]]  # Encrypt refuses the empty message
    msgs, pubs, sks, ephs, ivs, s2s, cts = (list(x) for x in zip(*it))
    n = len(it)
    e = DevEncrypt(ctx, msgs, pubs, ephs, ivs, s2s, base=0)
    d = DevDecrypt(ctx, [bytes(len(c)) for c in cts], sks, s2s, base=0)  # placeholders: ct comes from Encrypt
    torch.cuda.synchronize()
    cs = torch.cuda.Stream()
    with torch.cuda.stream(cs):
        e.run(cs)
        d.d_ct = e.d_ct  # item i at msg_off[i] + 113 i: the ciphertexts lie back to back
        d.d_off = e.d_off + OV * torch.arange(n + 1, device=e.d_off.device, dtype=torch.int64)
        d.run(cs)
    cs.synchronize()
    e.check([(0, c) for c in cts])
    d.check([(0, m) for m in msgs])


# ---------------------------------------------------------------- 5. secret hygiene of the host forms
def test_staged_secrets_are_wiped(ctx, pool):
    """after each host form returns, the arena's secret extent (keys, work area, plaintext: first and
    contiguous from offset 0, tests/test_ecies_stage_host.py) holds nothing; the public buffer behind it
    still holds its input, so the read looks at the arena this call staged in"""
    def al(b):
        return (max(b, 1) + 255) // 256 * 256
    it = pool[:100]
    msgs, pubs, sks, ephs, ivs, s2s, cts = (list(x) for x in zip(*it))
    n = len(it)
    flat_ct, flat_msg = b"".join(cts), b"".join(msgs)
    got, st = ctx.ecies_decrypt_batch(cts, u8(b"".join(sks), 32), s2s)
    assert not st.any() and got == msgs
    secret = al(n * 32) + al(n * 113) + al(len(flat_ct))
    assert not ctx._arena_read(0, secret).any(), "keys, Ke || Km or plaintext left in the arena"
    assert bytes(ctx._arena_read(secret, len(flat_ct))) == flat_ct
    got, st = ctx.ecies_encrypt_batch(msgs, u8(b"".join(pubs), 64), u8(b"".join(ephs), 32), u8(b"".join(ivs), 16), s2s)
    assert got[0] == cts[0]
    secret = al(n * 32) + al(n * 115) + al(len(flat_msg))
    assert not ctx._arena_read(0, secret).any(), "ephemeral keys, Ke || Km or plaintext left in the arena"
    assert bytes(ctx._arena_read(secret, n * 64)) == b"".join(pubs)


# ---------------------------------------------------------------- 6. timing ids, capture
def test_dev_forms_are_timed_apart_and_capturable(ctx, pool):
    import torch
    from gsv import _lib
    it = pool[:65]
    msgs, pubs, sks, ephs, ivs, s2s, cts = (list(x) for x in zip(*it))
    want_d = [(0, m) for m in msgs]
    want_e = [(0, c) if m else (M.ST_INVALID_MESSAGE, bytes(OV)) for m, c in zip(msgs, cts)]
    d, e = DevDecrypt(ctx, cts, sks, s2s), DevEncrypt(ctx, msgs, pubs, ephs, ivs, s2s)
    torch.cuda.synchronize()
    cs = torch.cuda.Stream()
    ctx.set_timing(True)
    try:
        ctx.reset_timing()
        d.run(cs)
        cs.synchronize()
        sym_ms, sym_launches = ctx.kernel_time(_lib.K_ECIES)
        lad_ms, lad_launches = ctx.kernel_time(_lib.K_ECRECOVER)
        assert sym_launches == 1 and lad_launches == 1 and sym_ms > 0 and lad_ms > 0
        e.run(cs)
        cs.synchronize()
        assert ctx.kernel_time(_lib.K_ECIES)[1] == 2 and ctx.kernel_time(_lib.K_ECRECOVER)[1] == 2
    finally:
        ctx.set_timing(False)
        ctx.reset_timing()
    d.check(want_d)
    e.check(want_e)
    # captured on an explicit stream (nothing allocated, nothing synchronised inside), replayed twice
    g = torch.cuda.CUDAGraph()
    shapes_before = ctx.prepared_shapes()
    with torch.cuda.graph(g, stream=cs):
        d.run(cs)
        e.run(cs)
    assert ctx.prepared_shapes() == shapes_before
    for _ in range(2):
        for t in (d.d_msg, d.d_st, d.d_work, e.d_ct, e.d_st, e.d_work):
            t.fill_(GUARD)
        d.d_mlen.fill_(0x6EEEEEEE)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        d.check(want_d)
        e.check(want_e)


# ---------------------------------------------------------------- 7. launch-shape edges
def test_empty_batch_and_argument_errors(ctx):
    from gsv import _lib
    L = _lib.load()
    h = ctx.handle
    msgs, st = ctx.ecies_decrypt_batch([], np.zeros((0, 32), np.uint8))
    assert msgs == [] and st.shape == (0,)
    msgs, st = ctx.ecies_encrypt_batch([], np.zeros((0, 64), np.uint8), np.zeros((0, 32), np.uint8),
                                       np.zeros((0, 16), np.uint8))
    assert msgs == [] and st.shape == (0,)
    assert L.gsv_ecies_decrypt_batch(h, None, None, None, None, None, 0, None, None, None) == 0
    assert L.gsv_ecies_encrypt_batch(h, None, None, None, None, None, None, None, 0, None, None) == 0
    assert L.gsv_ecies_decrypt_batch_dev(h, None, None, None, None, None, 0, None, None, None, None, None) == 0
    assert L.gsv_ecies_encrypt_batch_dev(h, None, None, None, None, None, None, None, 0, None, None, None, None) == 0
    buf = np.zeros(256, np.uint8)
    p = buf.ctypes.data
    off = np.array([0, 120], np.uint64)
    po = off.ctypes.data
    E = _lib.E_INVALID_ARG
    dec = [p, po, p, None, None, 1, p, p, p]
    enc = [p, po, p, p, p, None, None, 1, p, p]
    for k in (0, 1, 2, 6, 7, 8):
        a = list(dec)
        a[k] = None
        assert L.gsv_ecies_decrypt_batch(h, *a) == E, k
        assert L.gsv_ecies_decrypt_batch_dev(h, *a, p, None) == E, k
    assert L.gsv_ecies_decrypt_batch_dev(h, *dec, None, None) == E
    for k in (0, 1, 2, 3, 4, 8, 9):
        a = list(enc)
        a[k] = None
        assert L.gsv_ecies_encrypt_batch(h, *a) == E, k
        assert L.gsv_ecies_encrypt_batch_dev(h, *a, p, None) == E, k
    assert L.gsv_ecies_encrypt_batch_dev(h, *enc, None, None) == E
    # one empty ciphertext and one one-byte ciphertext: defined statuses through the host form
    msgs, st = ctx.ecies_decrypt_batch([b"", b"\x09"], np.ones((2, 32), np.uint8))
    assert msgs == [b"", b""] and list(st) == [_lib.ST_INVALID_MESSAGE, _lib.ST_INVALID_PUBKEY]
