"""Mirror of the reference's core/types signing entry points, batched on the GPU.

    EIP155Signer(chainId)        core/types/transaction_signing.go:108-125
    HomesteadSigner()            :169-180
    FrontierSigner()             :186-193
    SignTx(tx, signer, prv)      :56-63: signer.Hash(tx), crypto.Sign, tx.WithSignature
    SignTxBatch(txs, signer, keys)   batch form: per-item status codes

    HeaderHashes(rlps)           Header.Hash() and Header.HashNoNonce() (core/types/block.go:99-122) over a batch

The inverse, types.Sender over a batch, is Context.tx_sender_batch with the signer's kind and chain_id.
Transactions travel as their RLP encoding (rlp.EncodeToBytes(tx)), signed or not; an unsigned
NewTransaction carries V = R = S = 0.
"""
from __future__ import annotations

import numpy as np

from . import _lib, default_context
from .crypto import ErrInvalidKey, _padded_key


class ErrBadRLP(ValueError):
    """rlp: the transaction does not decode"""


class _Signer:
    kind = None
    chain_id = 0

    def __eq__(self, other):  # Signer.Equal
        return isinstance(other, _Signer) and (self.kind, self.chain_id) == (other.kind, other.chain_id)

    def __hash__(self):
        return hash((self.kind, self.chain_id))


class EIP155Signer(_Signer):
    """NewEIP155Signer(chainId): a nil chain id is 0 (transaction_signing.go:113-121)"""
    kind = _lib.SIGNER_EIP155

    def __init__(self, chain_id=None):
        self.chain_id = int(chain_id or 0)
        if self.chain_id < 0 or self.chain_id >> 512:
            raise ValueError("the chain id is a non-negative integer of at most 64 bytes")


class HomesteadSigner(_Signer):
    kind = _lib.SIGNER_HOMESTEAD


class FrontierSigner(_Signer):
    kind = _lib.SIGNER_FRONTIER


def SignTxBatch(txs, signer, keys, want_hash=True, ctx=None):
    """Batch types.SignTx: txs = RLP-encoded transactions, keys = one secret key each (an int, or up to 32
    big-endian bytes).  Returns (signed: list of bytes, b"" for a failed item; hashes (n,32) uint8 tx.Hash()
    or None; status (n,)).  A key with no 32-byte form raises ErrInvalidKey before anything is signed."""
    rows = np.frombuffer(b"".join(_padded_key(k) for k in keys), np.uint8).reshape(-1, 32)
    return (ctx or default_context()).tx_sign_batch([bytes(t) for t in txs], rows, signer.chain_id, signer.kind,
                                                    want_hash=want_hash)


def SignTx(tx_rlp: bytes, signer, prv, ctx=None) -> bytes:
    """types.SignTx (core/types/transaction_signing.go:56-63): the RLP of `tx_rlp`'s transaction signed by
    `prv` under `signer`, byte for byte the reference's.  ErrBadRLP where rlp.DecodeBytes refuses the
    input, ErrInvalidKey where crypto.Sign refuses the key."""
    signed, _, st = SignTxBatch([tx_rlp], signer, [prv], want_hash=False, ctx=ctx)
    if st[0] == _lib.ST_INVALID_KEY:
        raise ErrInvalidKey("invalid private key")
    if st[0] == _lib.ST_BODY_TOO_LARGE:
        raise ValueError(_lib.STATUS_STRINGS[_lib.ST_BODY_TOO_LARGE])
    if st[0] != _lib.ST_OK:
        raise ErrBadRLP(_lib.STATUS_STRINGS[_lib.ST_BAD_RLP])
    return signed[0]


def HeaderHashes(rlps, ctx=None):
    """Header.Hash() and Header.HashNoNonce() of RLP-encoded headers (rlp.EncodeToBytes(header)): (hashes (n, 32)
    uint8, hashes without nonce (n, 32) uint8, status (n,): ST_OK, ST_BAD_RLP where rlp.DecodeBytes refuses the
    header, ST_HEADER_TOO_WIDE for a Difficulty or Time above 32 bytes or a Number above 8).  Both rows of a header
    with ST_BAD_RLP are zeros."""
    return (ctx or default_context()).block_header_hash_batch(rlps)


__all__ = ["HeaderHashes", "EIP155Signer", "HomesteadSigner", "FrontierSigner", "SignTx", "SignTxBatch", "ErrInvalidKey", "ErrBadRLP"]
