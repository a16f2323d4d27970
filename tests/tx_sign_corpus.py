"""TEST INFRASTRUCTURE — the seeded transaction sets of tests/test_tx_sign_cpu.py, tests/test_gpu_tx_sign.py
and tests/golden/make_tx_sign_golden.py, and their expected results from tests/tx_sign_model.py with the
reference's own signer (oracle.ref().gsvref_sign) and oracle.keccak256.  Deterministic: fixed seeds."""
from __future__ import annotations

import ctypes
import random

import tx_rules_model as M
import tx_sign_model as S

N = M.SECP_N
C32 = int.from_bytes(bytes(range(0x81, 0x81 + 32)), "big")  # a 32-byte chain id
C64 = int.from_bytes(bytes(range(0x41, 0x41 + 64)), "big")  # a 64-byte one: V's item takes the long-string header
C64T = int.from_bytes(bytes(range(0xA1, 0xA1 + 64)), "big")  # its top bit set: V has 65 bytes, the longest item
# 46: V = 127 / 128 (one recid a single byte, the other 81 80); 110: V = 255 / 256; 2^63 - 18: V reaches 2^64
CHAIN_IDS = (0, 1, 46, 110, 2 ** 63 - 18, 2 ** 63 + 5, C32, C64, C64T)


def sender_is_inverse(signer, chain_id):
    """Does types.Sender under the same signer give the signing key's address back?  Not for EIP155Signer
    with chain id 0, in the reference itself: SignatureValues leaves V = 27 / 28 (transaction_signing.go:146)
    over a hash that carries chainId = 0 (:155-165), and Sender reads such a V as unprotected and recovers
    over the six-field hash (:128-130).  And not, in this project's three Sender decoders, for a chain id of
    2^511 or more: they refuse a V longer than 64 bytes as ErrInvalidChainId (csrc/notary.hip v_big_path)."""
    return not (signer == M.SIGNER_EIP155 and (chain_id == 0 or chain_id >> 511))


def signer_address(O, signed: bytes, signer, chain_id):
    """the address whose key made `signed`'s signature over the hash types.SignTx signed (the signer's own
    Hash), by oracle.ecrecover: the pin where sender_is_inverse is False"""
    tx = M.decode_txdata(signed)
    recid = tx["v"] - (35 + 2 * chain_id if signer == M.SIGNER_EIP155 and chain_id else 27)
    rc, pub = O.ecrecover(O.keccak256(S.sighash_pre(tx, signer, chain_id)),
                          tx["r"].to_bytes(32, "big") + tx["s"].to_bytes(32, "big") + bytes([recid]))
    return O.keccak256(pub[1:])[12:] if rc == 1 else None
# (signer, chain id) of every call: EIP-155 under each chain id, the two others once
GROUPS = tuple((M.SIGNER_EIP155, c) for c in CHAIN_IDS) + ((M.SIGNER_HOMESTEAD, 1), (M.SIGNER_FRONTIER, 1))
NONCES = (0, 1, 127, 128, 2 ** 64 - 1)
DATA_LENS = (0, 1, 55, 56, 255, 256, 1100)
BLOCK_EDGES = (135, 136, 137, 271, 272, 273)  # around one and two Keccak rate blocks
TO = bytes(range(0x31, 0x31 + 20))


def be(x: int) -> bytes:
    return x.to_bytes((x.bit_length() + 7) // 8, "big") if x else b""


def ref_signer(O):
    """(msg32, key32) -> 65 bytes by the reference's libsecp256k1 (RFC 6979 nonce), None for a refused key"""
    R = O.ref()
    assert R is not None, "the reference build oracle/_ref is needed (built by __graft_entry__.build())"

    def sign(msg32, key32):
        out = ctypes.create_string_buffer(65)
        return out.raw if R.gsvref_sign(out, msg32, key32) == 1 else None
    return sign


def model_signer(O):
    """the same signatures without the reference build: the oracle's signer with tests/rfc6979_model.py's
    nonce (tests/test_rfc6979_cpu.py ties both to the reference)"""
    import rfc6979_model as F

    def sign(msg32, key32):
        return O.secp_sign(msg32, key32, F.nonce(key32, msg32))
    return sign


def fixture_inputs(O, short):
    """[(label, blob, key32, signer, chain_id)] of tests/golden/tx_sign.json; `short` = find_short's result"""
    rng = random.Random(0x60_1d)
    rows = []
    key = lambda: be(rng.randrange(1, N)).rjust(32, b"\0")
    for name, blob in short.items():
        rows.append((name, blob, SEARCH_KEY, M.SIGNER_EIP155, 1))
    shapes = [("to20", dict(to=TO, data=b""), False), ("create", dict(to=None, data=b"\x60\x00"), False),
              ("create c0", dict(to=None, data=b"\x7f"), True), ("data 55", dict(to=TO, data=_data(rng, 55)), False),
              ("data 56", dict(to=TO, data=_data(rng, 56)), False), ("data 300", dict(to=None, data=_data(rng, 300)), True)]
    for signer, cid in GROUPS:
        for j, (name, f, as_list) in enumerate(shapes):
            f = dict(nonce=NONCES[(j + cid) % 5], price=_rand_int(rng, (7 * j + cid) % 33), gas=21000 + j,
                     value=_rand_int(rng, (5 * j) % 33), **f)
            blob, k = _blob(f, as_list), key()
            rows.append(("%s signer %d chain %d" % (name, signer, cid), blob, k, signer, cid))
    # the same transaction already signed (by another key, for another chain): re-signed, same output
    sign = model_signer(O)
    for label, blob, k, signer, cid in list(rows[len(short):len(short) + 12]):
        st, signed, _ = S.sign_tx(blob, key(), M.SIGNER_EIP155, 5, sign, O.keccak256)
        assert st == S.ST_OK
        rows.append((label + ", signed before", signed, k, signer, cid))
    # failures: what does not decode, the key rule, both at once
    good = S.unsigned_tx(9, 20 * 10 ** 9, 21000, TO, 10 ** 18, b"")
    pay = good[1:]  # a payload below 56 bytes: a one-byte list header
    assert good[0] == 0xC0 + len(pay) and pay[0] == 9
    bad_rlp = [("empty", b""), ("a string", M.enc_string(pay)), ("eight items", M.enc_list(pay[:-1])),
               ("trailing byte", good + b"\x00"), ("nonce 00", M.enc_list(b"\x00" + pay[1:])),
               ("V with a leading zero", M.enc_list(pay[:-3] + b"\x82\x00\x1b\x80\x80"))]
    for name, blob in bad_rlp:
        rows.append(("bad rlp: " + name, blob, key(), M.SIGNER_EIP155, 1))
    for kv in (0, N, 2 ** 256 - 1):
        rows.append(("key %x" % kv, good, kv.to_bytes(32, "big"), M.SIGNER_EIP155, 1))
    rows.append(("bad rlp and key 0", good + b"\x00", bytes(32), M.SIGNER_HOMESTEAD, 1))
    return rows


def _rand_int(rng, nbytes):
    """a value of exactly nbytes bytes (0 for nbytes = 0)"""
    return 0 if nbytes == 0 else rng.randrange(1 << (8 * nbytes - 8), 1 << (8 * nbytes))


def _data(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


def _fields(rng, k):
    """the six fields of transaction k of a group: every axis of the issue's table cycles"""
    to = (TO, None, None)[k % 3]
    d = DATA_LENS[(k // 3) % len(DATA_LENS)]
    data = _data(rng, d)
    if d == 1:
        data = bytes([0x7f if (k // 21) % 2 else 0x80])  # a byte below and at 0x80
    return dict(nonce=NONCES[k % len(NONCES)], price=_rand_int(rng, rng.randrange(0, 33)),
                gas=_rand_int(rng, rng.randrange(0, 9)), to=to, value=_rand_int(rng, rng.randrange(0, 33)),
                data=data), (to is None and k % 3 == 2)


def _blob(f, as_list):
    return S.unsigned_tx(f["nonce"], f["price"], f["gas"], f["to"], f["value"], f["data"], as_list)


def _signed_len(f, as_list, vlen):
    """length of the signed encoding when V's item has vlen bytes and R, S 32 bytes each"""
    b = _blob(f, as_list)
    payload = len(b) - (1 if b[0] < 0xF8 else 1 + b[0] - 0xF7) - 3 + vlen + 66
    return len(M.enc_head(payload, 0xC0, 0xF7)) + payload


def _fit(f, as_list, measure, target):
    """lengthen or shorten the data until measure(fields) == target (None if no length does)"""
    for _ in range(8):
        got = measure(f)
        if got == target:
            return True
        d = len(f["data"]) + target - got
        if d < 0:
            return False
        f["data"] = bytes((11 * j + 5) & 0xFF or 1 for j in range(d))
    return False


def differential(count=4096, seed=0x7a51):
    """[(blob, key32, signer, chain_id)], grouped by GROUPS in order"""
    rng = random.Random(seed)
    per = count // len(GROUPS)
    out = []
    for g, (signer, cid) in enumerate(GROUPS):
        n = per + (count - per * len(GROUPS) if g == 0 else 0)
        vlen = len(M.enc_uint(35 + 2 * cid + 1)) if signer == M.SIGNER_EIP155 and cid else 1
        items = []
        for k in range(n):
            f, as_list = _fields(rng, k)
            # Keccak block boundaries: the sighash preimage, then the signed encoding (R, S of 32 bytes,
            # which all but 1 in 128 are), put on each edge
            edge = BLOCK_EDGES[(k // 16) % 6]
            if k % 16 == 5:
                _fit(f, as_list, lambda x: len(S.sighash_pre(x, signer, cid)), edge)
            elif k % 16 == 11:
                _fit(f, as_list, lambda x: _signed_len(x, as_list, vlen), edge)
            elif k % 16 == 7:  # list header: an input payload of 55 / 255 bytes and below grows past it
                f["price"], f["value"], f["gas"] = 0, 0, 0
                _fit(f, as_list, lambda x: len(_blob(x, as_list)), (40, 56, 250, 257)[(k // 16) % 4])
            items.append((_blob(f, as_list), be(rng.randrange(1, N)).rjust(32, b"\0"), signer, cid))
        out += items
    return out


def expected(O, items):
    """[(status, signed, hash)] by the model with the reference's signer"""
    sign = ref_signer(O)
    return [S.sign_tx(b, k, s, c, sign, O.keccak256) for b, k, s, c in items]


SEARCH_KEY = (7).to_bytes(32, "big")
# the classes of short signature halves the fixture must hold: predicate over (bytes of R, bytes of S)
SHORT_CLASSES = (("R of 31 bytes", lambda rl, sl: rl == 31), ("S of 31 bytes", lambda rl, sl: sl == 31),
                 ("R or S of at most 30 bytes", lambda rl, sl: min(rl, sl) <= 30))


def sig_lens(signed: bytes):
    """(bytes of R, bytes of S) of a signed transaction"""
    tx = M.decode_txdata(signed)
    return len(be(tx["r"])), len(be(tx["s"]))


def find_short(O, limit=1 << 20):
    """{class name: blob}: for each of SHORT_CLASSES the first transaction (nonce counted up from 0, chain id
    1, EIP-155, SEARCH_KEY) whose signature falls in it; at most `limit` signatures are made, and a class
    nothing fell in is absent"""
    sign = ref_signer(O)
    found = {}
    for j in range(limit):
        blob = S.unsigned_tx(j, 20 * 10 ** 9, 21000, TO, 10 ** 18, b"")
        sig = sign(O.keccak256(S.sighash_pre(M.decode_txdata(blob), M.SIGNER_EIP155, 1)), SEARCH_KEY)
        rl, sl = len(be(int.from_bytes(sig[:32], "big"))), len(be(int.from_bytes(sig[32:64], "big")))
        for name, pred in SHORT_CLASSES:
            if name not in found and pred(rl, sl):
                found[name] = blob
        if len(found) == len(SHORT_CLASSES):
            break
    return found
