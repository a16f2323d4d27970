"""Mirror of the reference's core/types signing entry points, batched on the GPU.

    EIP155Signer(chainId)        core/types/transaction_signing.go:108-125
    HomesteadSigner()            :169-180
    FrontierSigner()             :186-193
    SignTx(tx, signer, prv)      :56-63: signer.Hash(tx), crypto.Sign, tx.WithSignature
    SignTxBatch(txs, signer, keys)   batch form: per-item status codes

    HeaderHashes(rlps)           Header.Hash() and Header.HashNoNonce() (core/types/block.go:99-122) over a batch

    Bloom9(items)                bloom9 / calcBloomIndexes (core/types/bloom9.go:115-127): three bit numbers each
    BloomLookup(bloom, topic)    :131-136; BloomLookupBatch(blooms, topics) over pairs
    LogsBloom(receipt_rlps)      :103-113 per RLP-encoded receipt
    CreateBloom(receipt_rlps)    :94-101 over one list; CreateBloomBatch(lists) over many

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


BloomByteLength = 256  # bloom9.go:33


class ErrBadReceipt(ValueError):
    """a receipt that rlp.DecodeBytes refuses, or whose status field setStatus refuses (receipt.go:116-128)"""


def Bloom9(items, ctx=None):
    """bloom9 of each byte string (bloom9.go:115-127) as its three bit numbers: (n, 3) uint16, bit b being byte
    255 - b // 8 under mask 1 << (b % 8) of a Bloom."""
    return (ctx or default_context()).bloom9_batch(items)


def _bloom_rows(blooms):
    rows = np.frombuffer(b"".join(bytes(b) for b in blooms), np.uint8).reshape(len(blooms), -1)
    if rows.shape[0] and rows.shape[1] != BloomByteLength:
        raise ValueError("a Bloom is 256 bytes")
    return rows.reshape(-1, BloomByteLength)


def BloomLookupBatch(blooms, topics, ctx=None):
    """BloomLookup(blooms[i], topics[i]) (bloom9.go:131-136): (n,) bool; the hashes run on the GPU, the three bit
    tests per pair on the host."""
    rows = _bloom_rows(blooms)
    idx = Bloom9(topics, ctx).astype(np.int64)
    if idx.shape[0] != rows.shape[0]:
        raise ValueError("one topic per bloom")
    k = np.arange(rows.shape[0])[:, None]
    return ((rows[k, 255 - (idx >> 3)] >> (idx & 7)) & 1).all(axis=1)


def BloomLookup(bloom, topic, ctx=None) -> bool:
    return bool(BloomLookupBatch([bloom], [topic], ctx)[0])


def CreateBloomBatch(lists, ctx=None):
    """types.CreateBloom (bloom9.go:94-101) of each list of RLP-encoded receipts: (blooms (n, 256) uint8, status
    (n,): ST_OK, or the first failing receipt's ST_BAD_RLP / ST_RECEIPT_STATUS with a zero row)."""
    st, _, bloom, _, _ = (ctx or default_context()).receipts_verify_batch(lists)
    return bloom, st


def CreateBloom(receipt_rlps, ctx=None) -> bytes:
    """types.CreateBloom over one block's receipts; ErrBadReceipt where one of them does not decode"""
    bloom, st = CreateBloomBatch([receipt_rlps], ctx)
    if st[0] != _lib.ST_OK:
        raise ErrBadReceipt(_lib.STATUS_STRINGS[int(st[0])])
    return bloom[0].tobytes()


def LogsBloom(receipt_rlps, ctx=None):
    """types.LogsBloom(receipt.Logs) (bloom9.go:103-113) per RLP-encoded receipt: (rows (n, 256) uint8, status (n,))"""
    return CreateBloomBatch([[r] for r in receipt_rlps], ctx)


__all__ = ["Bloom9", "BloomLookup", "BloomLookupBatch", "LogsBloom", "CreateBloom", "CreateBloomBatch", "ErrBadReceipt",
           "HeaderHashes", "EIP155Signer", "HomesteadSigner", "FrontierSigner", "SignTx", "SignTxBatch", "ErrInvalidKey", "ErrBadRLP"]
