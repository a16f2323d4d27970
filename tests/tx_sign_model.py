"""TEST INFRASTRUCTURE — a pure-Python model of types.SignTx over RLP-encoded transactions, built from
tests/tx_rules_model.py's decode_txdata, enc_* and sighash_preimage, written from the reference's Go text
and independent of the code under test (csrc/txsign.hip, csrc/gsv_txsign.hip): no import of `gsv`.

    sign_tx     core/types/transaction_signing.go:56-63 SignTx: h = s.Hash(tx), sig = crypto.Sign(h, prv),
                tx.WithSignature(s, sig)
    sig_values  :141-151 EIP155Signer.SignatureValues, :195-203 FrontierSigner.SignatureValues
    encode_tx   rlp.Encode of txdata (core/types/transaction.go:55-70), tx.Hash() = keccak of it (:198-206)

The signature itself is not modelled: `sign` is a callable (msg32, key32) -> 65 bytes [R || S || recid] or
None for a key the signer refuses; the tests pass the reference's own signer (oracle.ref().gsvref_sign) and
oracle.keccak256.
"""
from __future__ import annotations

import tx_rules_model as M

ST_OK, ST_BAD_RLP, ST_INVALID_KEY, ST_BODY_TOO_LARGE = 0, 8, 11, 13
MAX_ITEM = 1 << 20  # the one documented deviation: a longer item is not signed
N = M.SECP_N


def key_ok(key32: bytes) -> bool:  # secp256k1_ec_seckey_verify (crypto/secp256k1/secp256.go:78)
    return 0 < int.from_bytes(key32, "big") < N


def sighash_pre(tx, signer, chain_id):
    """the bytes the signer's Hash hashes: EIP155Signer.Hash carries chainId, 0, 0 even when chainId is 0"""
    return M.sighash_preimage(tx, chain_id if signer == M.SIGNER_EIP155 else None)


def sig_values(sig65: bytes, signer, chain_id):
    """(R, S, V) as big integers"""
    r, s = int.from_bytes(sig65[:32], "big"), int.from_bytes(sig65[32:64], "big")
    v = sig65[64] + 27
    if signer == M.SIGNER_EIP155 and chain_id != 0:
        v = sig65[64] + 35 + 2 * chain_id
    return r, s, v


def encode_tx(tx) -> bytes:
    """rlp.Encode of the nine fields, a nil recipient as 0x80"""
    return M.enc_list(M.enc_uint(tx["nonce"]) + M.enc_uint(tx["price"]) + M.enc_uint(tx["gas"]) +
                      (b"\x80" if tx["to"] is None else M.enc_string(tx["to"])) + M.enc_uint(tx["value"]) +
                      M.enc_string(tx["data"]) + M.enc_uint(tx["v"]) + M.enc_uint(tx["r"]) + M.enc_uint(tx["s"]))


def sign_tx(blob: bytes, key32: bytes, signer, chain_id, sign, keccak):
    """(status, signed RLP, tx hash): b"" and 32 zero bytes for a failed item.  The reference decodes
    before it signs, so ST_BAD_RLP comes before ST_INVALID_KEY."""
    fail = b"", bytes(32)
    if len(blob) > MAX_ITEM:
        return (ST_BODY_TOO_LARGE,) + fail
    try:
        tx = M.decode_txdata(blob)
    except M.RLPError:
        return (ST_BAD_RLP,) + fail
    if not key_ok(key32):
        return (ST_INVALID_KEY,) + fail
    sig = sign(keccak(sighash_pre(tx, signer, chain_id)), key32)
    assert sig is not None and len(sig) == 65
    tx = dict(tx)
    tx["r"], tx["s"], tx["v"] = sig_values(sig, signer, chain_id)
    out = encode_tx(tx)
    return ST_OK, out, keccak(out)


def growth(chain_id_len: int) -> int:
    """GSV_TX_SIGN_GROWTH as include/gsv.h derives it: header + 1, V chain_id_len + 3 against 1, R and S 33
    against 1 each"""
    return 1 + (chain_id_len + 3 - 1) + 2 * (33 - 1)


def unsigned_tx(nonce, price, gas, to, value, data, to_as_list=False) -> bytes:
    """rlp.EncodeToBytes(NewTransaction(...)): V = R = S = 0.  to_as_list sends a nil recipient as 0xc0,
    which only a decoder following rlp/decode.go:486-496 accepts"""
    rcpt = (b"\xc0" if to_as_list else b"\x80") if to is None else M.enc_string(to)
    return M.enc_list(M.enc_uint(nonce) + M.enc_uint(price) + M.enc_uint(gas) + rcpt + M.enc_uint(value) +
                      M.enc_string(data) + b"\x80\x80\x80")
