"""TEST INFRASTRUCTURE — the structured transaction corpus of tests/test_tx_rules.py (CPU) and
tests/test_gpu_tx_rules.py (GPU), and its expected results from tests/tx_rules_model.py.

Deterministic: one fixed key, fixed seeds.  Signed base transactions (20-byte recipient and contract
creation, EIP-155 and unprotected); every one of the nine fields replaced by every encoding of SUBS;
outer-level damage; V values and widths; positive cases that only a decoder following rlp/decode.go
accepts; each placed as is and shifted so that the replaced item's first byte is the last data byte of a
31-byte chunk (the next byte read through the chunk map then lies across an indicator byte).
"""
from __future__ import annotations

import hashlib
import random

import tx_rules_model as M

KEY = bytes.fromhex("4c0883a69102937d6231471b5dbb6204fe5129617082792ae468d01a3f362318")
CHAIN_IDS = (0, 1, 2 ** 63 + 5)
SIGNERS = (M.SIGNER_EIP155, M.SIGNER_HOMESTEAD, M.SIGNER_FRONTIER)
FIELDS = ("nonce", "price", "gas", "to", "value", "data", "v", "r", "s")
ALL_STATUSES = {M.ST_OK, M.ST_BAD_RLP, M.ST_INVALID_SIG, M.ST_INVALID_CHAIN_ID, M.ST_RECOVER_FAILED}
TO = bytes(range(0x31, 0x31 + 20))


def _rand(rng, n):
    """n random bytes whose first is >= 0x80: a canonical integer and never a lone single byte"""
    return bytes([0x80 | rng.getrandbits(7)] + [rng.getrandbits(8) for _ in range(n - 1)]) if n else b""


def subs(rng):
    """(label, encoding) of the issue's list, plus two size-field extremes"""
    out = [("80", b"\x80"), ("00", b"\x00"), ("01", b"\x01"), ("7f", b"\x7f"),
           ("8100", b"\x81\x00"), ("817f", b"\x81\x7f"), ("8180", b"\x81\x80"),
           ("2 bytes, leading zero", b"\x82\x00\x05")]
    for n in (8, 9, 20, 21, 32, 33, 55):
        out.append((f"{n} bytes", bytes([0x80 + n]) + _rand(rng, n)))
    out += [("56 bytes, long form", b"\xb8\x38" + _rand(rng, 56)),
            ("56 bytes, two-byte length", b"\xb9\x00\x38" + _rand(rng, 56)),
            ("long form announcing 55", b"\xb8\x37" + _rand(rng, 55)),
            ("256 bytes", b"\xb9\x01\x00" + _rand(rng, 256)),
            ("257 bytes", b"\xb9\x01\x01" + _rand(rng, 257)),
            ("5000 bytes", b"\xb9\x13\x88" + _rand(rng, 5000)),
            ("c0", b"\xc0"), ("c101", b"\xc1\x01"),
            ("long list", b"\xf8\x38" + b"\x01" * 56),
            # not in the issue's list: a length of 2^64 - 1 (TestStreamKind's BFFF..FF row) overflows a
            # size check written as a sum, and a long string whose announced size passes the list's end
            ("long form announcing 2^64-1", b"\xbf" + b"\xff" * 8),
            ("long form past the list", b"\xb8\xff" + _rand(rng, 56))]
    return out


class Case:
    __slots__ = ("blob", "label", "positive")

    def __init__(self, blob, label, positive=None):
        self.blob, self.label, self.positive = blob, label, positive  # positive: None / "eip155" / "plain"


_SIGS = {}


def _sign(O, six, chain_id, eip155, k=7):
    """V, R, S items over the six items as the reference would hash them"""
    pre = M.enc_list(b"".join(six) + (M.enc_uint(chain_id) + b"\x80\x80" if eip155 else b""))
    if pre not in _SIGS:
        sig = O.secp_sign(O.keccak256(pre), KEY, k.to_bytes(32, "big"))
        v = sig[64] + (35 + 2 * chain_id if eip155 else 27)
        _SIGS[pre] = (M.enc_uint(v), M.enc_uint(int.from_bytes(sig[:32], "big")),
                      M.enc_uint(int.from_bytes(sig[32:64], "big")))
    return list(_SIGS[pre])


def _six(nonce, to, data, price=None):
    return [M.enc_uint(nonce), price if price is not None else M.enc_uint(20 * 10 ** 9), M.enc_uint(21000),
            b"\x80" if to is None else M.enc_string(to), M.enc_uint(10 ** 18 + nonce), M.enc_string(data)]


def _offset(items, i):
    """blob offset of item i's first byte"""
    total = sum(len(x) for x in items)
    return len(M.enc_head(total, 0xC0, 0xF7)) + sum(len(x) for x in items[:i])


def _placed(O, nonce, to, chain_id, eip155, i, repl, shift):
    """The nine items of a base transaction signed with KEY, item i replaced by `repl` after signing.
    shift: lengthen the payload (for V, R, S) or the gas price (for gas .. data; a *big.Int of any length
    is valid, rlp/decode.go:271-287) until the replaced item starts at blob offset 30 mod 31.  nonce and
    gas price start within the first 5 bytes and cannot be moved there; for them the payload is
    lengthened to a three-byte list header instead, which moves every item by one."""
    for pad in range(0, 80) if shift else (0,):
        data, price = b"\x05\x06\x07\x08\x09", None
        if shift and i >= 6:
            data = bytes((7 * j + 1) & 0xFF for j in range(5 + pad))
        elif shift and i >= 2:
            price = M.enc_string(bytes([0x81]) + bytes((3 * j + 2) & 0xFF for j in range(5 + pad)))
        elif shift:
            data = bytes((7 * j + 1) & 0xFF for j in range(300))
        six = _six(nonce, to, data, price)
        items = six + _sign(O, six, chain_id, eip155)
        if repl is not None:
            items[i] = repl
        if not shift or i < 2 or _offset(items, i) % 31 == 30:
            return items
    raise AssertionError("no padding puts the item at a chunk's last byte")


def build(O, chain_id, seed=20241019):
    """[Case] for one chain id (the EIP-155 bases are signed for it)."""
    rng = random.Random(seed)
    S = subs(rng)
    cases = []
    bases = [("to20", TO, True), ("create", None, True), ("to20", TO, False), ("create", None, False)]
    nonce = 0
    for shift in (False, True):
        sh = " shifted" if shift else ""
        for bname, to, eip155 in bases:
            kind = "eip155" if eip155 else "plain"
            nonce += 1
            # the untouched base is a positive case
            cases.append(Case(M.enc_list(b"".join(_placed(O, nonce, to, chain_id, eip155, 6, None, shift))),
                              f"base {bname} {kind}{sh}", kind))
            for i, fname in enumerate(FIELDS):
                for label, enc in S:
                    items = _placed(O, nonce, to, chain_id, eip155, i, enc, shift)
                    cases.append(Case(M.enc_list(b"".join(items)), f"{bname} {kind} {fname}={label}{sh}"))
            # V values and widths (R, S stay a valid signature of the base)
            vvals = [0, 1, 26, 27, 28, 29, 35, 36, 37, 38, 2 ** 64 - 1, 2 ** 64]
            vencs = [(str(v), M.enc_uint(v)) for v in vvals] + \
                    [(f"{n} bytes", M.enc_string(_rand(rng, n))) for n in (9, 33, 65, 300)]
            for label, enc in vencs:
                items = _placed(O, nonce, to, chain_id, eip155, 6, enc, shift)
                cases.append(Case(M.enc_list(b"".join(items)), f"{bname} {kind} V={label}{sh}"))
            # r = 2^255 + 2 is below n and no point has that x: ErrRecoverFailed-class (Ecrecover's error)
            items = _placed(O, nonce, to, chain_id, eip155, 7, M.enc_uint(2 ** 255 + 2), shift)
            cases.append(Case(M.enc_list(b"".join(items)), f"{bname} {kind} r off curve{sh}"))
            # outer level.  "shifted" here: the payload is lengthened until the blob ends at a chunk's
            # last data byte (the header is at offset 0 and cannot move), so a trailing byte opens a chunk
            for pad in range(0, 40) if shift else (0,):
                six = _six(nonce, to, bytes((5 * j + 3) & 0xFF for j in range(5 + pad)))
                items = six + _sign(O, six, chain_id, eip155)
                if not shift or len(M.enc_list(b"".join(items))) % 31 == 0:
                    break
            body = b"".join(items)
            good = M.enc_list(body)
            hdr = len(good) - len(body)
            lenb = lambda n: n.to_bytes(hdr - 1, "big")
            cases += [
                Case(M.enc_string(body), f"{bname} {kind} outer is a string{sh}"),
                Case(M.enc_list(b"".join(items[:8])), f"{bname} {kind} eight fields{sh}"),
                Case(M.enc_list(body + b"\x01"), f"{bname} {kind} ten fields{sh}"),
                Case(good[:1] + lenb(len(body) + 1) + body, f"{bname} {kind} outer length one too long{sh}"),
                Case(good[:1] + lenb(len(body) - 1) + body, f"{bname} {kind} outer length one too short{sh}"),
                Case(good + b"\x00", f"{bname} {kind} one trailing byte{sh}"),
            ]
            # a payload under 56 bytes: canonical short header (control) and the long form for it
            tiny = M.enc_uint(nonce) + b"\x01\x01\x80\x01\x80\x1b\x01\x01"
            cases += [Case(bytes([0xC0 + len(tiny)]) + tiny, f"{bname} {kind} tiny tx, short header{sh}"),
                      Case(b"\xf8" + bytes([len(tiny)]) + tiny,
                           f"{bname} {kind} tiny tx, long-form header under 56{sh}")]
            # positive cases only a decoder that follows rlp/decode.go accepts
            if to is None:  # recipient c0, signed over 80 (decode.go:486-496; the signer re-encodes nil as 80)
                items = _placed(O, nonce, None, chain_id, eip155, 3, b"\xc0", shift)
                cases.append(Case(M.enc_list(b"".join(items)), f"POSITIVE recipient c0 {kind}{sh}", kind))
            for f, fname in ((1, "price"), (4, "value")):
                for n in (257, 5000):
                    big = M.enc_string(_rand(rng, n))
                    for pad in range(0, 80) if shift else (0,):
                        six = _six(nonce, to, bytes((9 * j + 4) & 0xFF for j in range(pad)))
                        six[f] = big
                        items = six + _sign(O, six, chain_id, eip155)
                        if not shift or _offset(items, 6) % 31 == 30:  # V at a chunk's last byte
                            break
                    cases.append(Case(M.enc_list(b"".join(items)), f"POSITIVE {bname} {fname} of {n} bytes {kind}{sh}", kind))
    return cases


def positive_ok(case, signer):
    """Must this case give ST_OK with KEY's address?  An EIP-155 signature only under the EIP-155 signer
    (elsewhere V = 35 + 2c + recid is not 27/28); an unprotected one under all three (EIP155Signer hands
    it to HomesteadSigner, transaction_signing.go:128-130; s is low, so Frontier accepts it too)."""
    return case.positive == "plain" or (case.positive == "eip155" and signer == M.SIGNER_EIP155)


def key_address(O):
    return O.keccak256(O.secp_pubkey(KEY)[1:])[12:]


_EXPECT = {}


def expected(O, cases, chain_id, signer):
    """[(status, sender20 | None, model dict)] per case: the model's verdict, finished by oracle.ecrecover
    (the suite ties it to the reference's libsecp256k1) and the address Keccak."""
    h = hashlib.sha256()
    for c in cases:
        h.update(len(c.blob).to_bytes(4, "big") + c.blob)
    key = (chain_id, signer, h.digest())
    if key in _EXPECT:
        return _EXPECT[key]
    out = []
    for c in cases:
        st, d = M.tx_verdict(c.blob, signer, chain_id)
        addr = None
        if st == M.ST_OK:
            sig = d["r"].to_bytes(32, "big") + d["s"].to_bytes(32, "big") + bytes([d["v"]])
            rc, pub = O.ecrecover(O.keccak256(d["pre"]), sig)
            if rc == 1:
                addr = O.keccak256(pub[1:])[12:]
            else:
                st = M.ST_RECOVER_FAILED
        out.append((st, addr, d))
    _EXPECT[key] = out
    return out


# ---------------------------------------------------------------- blob-index bodies
def index_body(O, seed, chain_id=1):
    """One body of 40-70 KiB (more than 1,024 chunks: k_blob_index gives each thread a run of two or
    three) and a max_txs that cuts it off mid-way.  Returns (body, max_txs)."""
    rng = random.Random(seed)
    txs = []
    for j, n in enumerate((0, 1, 30, 31, 62, 120, 400, 1100)):
        six = _six(100 + j, TO if j % 2 else None, bytes(rng.getrandbits(8) for _ in range(n)))
        txs.append(M.enc_list(b"".join(six + _sign(O, six, chain_id, j % 3 != 0))))
    # one of each failing class: signed for another chain, r = 0, r = 2^255 + 2 (no point has that x)
    six = _six(200, TO, b"\x01\x02\x03")
    txs.append(M.enc_list(b"".join(six + _sign(O, six, chain_id + 4, True))))
    for r in (b"\x80", M.enc_uint(2 ** 255 + 2)):
        sig = _sign(O, six, chain_id, True)
        txs.append(M.enc_list(b"".join(six + [sig[0], r, sig[2]])))
    out = bytearray()

    def put(blob, ind_hi=0):
        n = (len(blob) + 30) // 31
        for j in range(n):
            part = blob[j * 31:(j + 1) * 31]
            term = j == n - 1
            # bits 5 and 6 are outside both masks (marshal.go:16-17): set them on some indicators
            ind = (len(part) if term else 0) | (ind_hi if term else ind_hi & 0x60)
            out.append(ind)
            out.extend(part + bytes(31 - len(part)))

    put(b"\xc0")                                   # a terminal chunk first, terminal length 1
    for k, t in enumerate(txs):                    # every transaction once, before any cut-off
        put(t, (0, 0x20, 0x80, 0xC0)[k % 4])
    want = rng.randrange(40, 70) * 1024
    big_done = False
    while len(out) < want:
        r = rng.random()
        hi = rng.choice((0, 0, 0x20, 0x40, 0x60, 0x80, 0xE0))   # bits 5/6, skipEvm (bit 7)
        if r < 0.55:
            put(rng.choice(txs), hi)
        elif r < 0.65:
            put(bytes(rng.getrandbits(8) for _ in range(31)), hi)          # terminal length 31
        elif r < 0.75:
            put(bytes(rng.getrandbits(8) for _ in range(1)), hi)           # terminal length 1
        elif r < 0.97 or big_done:
            put(bytes(rng.getrandbits(8) for _ in range(rng.randrange(1, 40 * 31))), hi)  # 1..40 chunks
        else:
            put(bytes(rng.getrandbits(8) for _ in range(31 * 12 + 5)), hi)  # longer than three threads' runs
            big_done = True
    if not big_done:
        put(bytes(rng.getrandbits(8) for _ in range(31 * 12 + 5)), 0x40)
        put(txs[3], 0x80)
    out += bytes(32 * 3)                           # non-terminal chunks last
    out += bytes(rng.getrandbits(8) for _ in range(rng.randrange(1, 32)))  # not a multiple of 32
    body = bytes(out)
    nblobs = len(M.deserialize(body))
    return body, max(8, (nblobs * 2 // 3) & ~7)
