"""Mirror of the reference's collation validation entry points (package sharding + types.DeriveSha),
batched on the GPU.

    DeriveSha(list)                  core/types/derive_sha.go:32-41 (any DerivableList: list of GetRlp(j))
    DeriveShaBatch(lists)            batch form: tx roots (core/block_validator.go:70), receipt roots (:92)
    CollationHeader.Hash()           sharding/collation.go:66-71
    Collation.CalculateChunkRoot()   sharding/collation.go:115-119
    Collation.CalculatePOC(salt)     sharding/collation.go:124-136
    VerifyProposerSignatures(hdrs)   proposer signature over the unsigned header hash, as made by
                                     SMCClient.Sign (sharding/mainchain/smc_client.go:245-248) at
                                     sharding/proposer/proposer.go:83 (the reference never checks it)
    SignHeaders(hdrs, keys)          that signature made: crypto.Sign over each unsigned header hash
    Serialize / Deserialize          sharding/utils/marshal.go:71-198 (the blob codec)
    SerializeTxToBlob / DeserializeBlobToTx   sharding/collation.go:158-206, over RLP-encoded transactions
    CreateCollations(...)            proposer.createCollation (sharding/proposer/proposer.go:55-92) as a batch

Integers (ShardID, Period) are Python ints (the reference's *big.Int); None stands for a nil pointer.
"""
from __future__ import annotations

import numpy as np

from . import _lib, default_context

COLLATION_SIZE_LIMIT = 1 << 20  # sharding/collation.go:45


class ErrProposerMismatch(ValueError):
    """recovered proposer signature address differs from the header's ProposerAddress"""


def DeriveSha(items, ctx=None) -> bytes:
    """types.DeriveSha over a list whose GetRlp(j) is items[j] (bytes)."""
    return bytes((ctx or default_context()).derive_sha_batch([list(items)])[0])


def DeriveShaBatch(lists, ctx=None) -> np.ndarray:
    return (ctx or default_context()).derive_sha_batch([list(x) for x in lists])


def _int32(x) -> bytes:
    x = 0 if x is None else int(x)
    if x < 0:
        raise ValueError("rlp: cannot encode negative *big.Int")
    return x.to_bytes(32, "big")


def _pack_headers(headers):
    n = len(headers)
    sid = np.zeros((n, 32), np.uint8)
    root = np.zeros((n, 32), np.uint8)
    per = np.zeros((n, 32), np.uint8)
    prop = np.zeros((n, 20), np.uint8)
    sig = np.zeros((n, 65), np.uint8)
    nil = np.zeros(n, np.uint8)
    for i, h in enumerate(headers):
        sid[i] = np.frombuffer(_int32(h.ShardID()), np.uint8)
        per[i] = np.frombuffer(_int32(h.Period()), np.uint8)
        if h.ChunkRoot() is None:
            nil[i] |= 1
        else:
            root[i] = np.frombuffer(bytes(h.ChunkRoot()), np.uint8)
        if h.ProposerAddress() is None:
            nil[i] |= 2
        else:
            prop[i] = np.frombuffer(bytes(h.ProposerAddress()), np.uint8)
        s = h.Sig()
        if not s:
            nil[i] |= 4
        elif len(s) != 65:
            raise ValueError("proposer signature must be 65 bytes [R || S || V]")
        else:
            sig[i] = np.frombuffer(bytes(s), np.uint8)
    return sid, root, per, prop, sig, nil


class CollationHeader:
    """sharding/collation.go:29-43 (collationHeaderData fields behind getters)."""

    def __init__(self, shard_id, chunk_root, period, proposer_address, proposer_signature=None):
        self._shard_id = shard_id
        self._chunk_root = None if chunk_root is None else bytes(chunk_root)
        self._period = period
        self._proposer = None if proposer_address is None else bytes(proposer_address)
        self._sig = None if proposer_signature is None else bytes(proposer_signature)

    def ShardID(self):
        return self._shard_id

    def Period(self):
        return self._period

    def ChunkRoot(self):
        return self._chunk_root

    def ProposerAddress(self):
        return self._proposer

    def Sig(self):
        return self._sig

    def AddSig(self, sig: bytes):
        self._sig = bytes(sig)

    def Hash(self, ctx=None) -> bytes:
        return bytes(HeaderHashBatch([self], ctx)[0])


def HeaderHashBatch(headers, ctx=None) -> np.ndarray:
    """CollationHeader.Hash() for each header (signature included as set)."""
    h, _, _ = (ctx or default_context()).collation_header_verify_batch(*_pack_headers(headers))
    return h


def VerifyProposerSignatures(headers, ctx=None):
    """-> (signers (n,20), status (n,)): GSV_ST_OK when the signature over the unsigned header hash
    recovers ProposerAddress, GSV_ST_PROPOSER_MISMATCH when it recovers another address, else the
    recovery status (crypto.Ecrecover errors).  A header without a signature (Sig() None or empty) is
    never recovered: GSV_ST_INVALID_SIG_LEN (secp256k1.ErrInvalidSignatureLen) and a zero signer."""
    _, signer, st = (ctx or default_context()).collation_header_verify_batch(*_pack_headers(headers))
    return signer, st


def SignHeaders(headers, keys, ctx=None):
    """The proposer's half of VerifyProposerSignatures: signs each header as createCollation does
    (sharding/proposer/proposer.go:83: SMCClient.Sign -> keystore.SignHash -> crypto.Sign over the
    header's hash with ProposerSignature empty) and AddSig's the 65-byte signature.  keys[i]: header i's
    secret key, an int or up to 32 big-endian bytes.  One batch of header hashes and one of signatures on
    the GPU.  A key that is no valid secret key raises crypto.ErrInvalidKey and leaves EVERY header as it
    was."""
    from . import crypto
    headers = list(headers)
    keys = [crypto._padded_key(k) for k in keys]
    if len(keys) != len(headers):
        raise ValueError("headers and keys batch sizes differ")
    if not headers:
        return
    unsigned = [CollationHeader(h.ShardID(), h.ChunkRoot(), h.Period(), h.ProposerAddress(), None) for h in headers]
    hashes = HeaderHashBatch(unsigned, ctx)
    sigs, st = crypto.SignBatch(hashes, np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 32), ctx)
    if (st != _lib.ST_OK).any():
        raise crypto.ErrInvalidKey("invalid private key (header %d)" % int(np.flatnonzero(st != _lib.ST_OK)[0]))
    for h, s in zip(headers, sigs):
        h.AddSig(bytes(s))


class Collation:
    """sharding/collation.go:15-27: header + serialized body."""

    def __init__(self, header: CollationHeader, body: bytes, transactions=None):
        self.header = header
        self.body = bytes(body)
        self.transactions = transactions

    def Header(self):
        return self.header

    def Body(self):
        return self.body

    def CalculateChunkRoot(self, ctx=None):
        root = bytes((ctx or default_context()).chunk_root_batch([self.body])[0])
        self.header._chunk_root = root

    def CalculatePOC(self, salt: bytes, ctx=None) -> bytes:
        return bytes((ctx or default_context()).collation_poc_batch([self.body], bytes(salt))[0])


def CalculatePOCBatch(bodies, salt: bytes, ctx=None) -> np.ndarray:
    return (ctx or default_context()).collation_poc_batch(list(bodies), bytes(salt))


# ---------------------------------------------------------------- the producer side
def Serialize(blobs, skip_evm=None, ctx=None) -> bytes:
    """utils.Serialize (sharding/utils/marshal.go:71-123): blobs = byte strings, skip_evm = their flags
    (None: all false).  A zero-length blob emits nothing, as in the reference.  No size limit."""
    blobs = [bytes(b) for b in blobs]
    if not blobs:
        return b""
    return (ctx or default_context()).blob_serialize_batch([blobs], None if skip_evm is None else [list(skip_evm)])[0]


def Deserialize(body, ctx=None):
    """utils.Deserialize (sharding/utils/marshal.go:144-198): the body's blobs as (bytes, skip_evm).  A
    body past 2^20 bytes is refused (GsvError, GSV_E_TOO_LARGE): no collation body is larger."""
    body = bytes(body)
    if len(body) < 32:
        return []
    return (ctx or default_context()).blob_deserialize_batch([body])[0]


def _size_error(size):
    return ValueError("the serialized body size %d exceeded the collation size limit %d" % (size, COLLATION_SIZE_LIMIT))


def SerializeTxToBlob(encoded_txs, ctx=None) -> bytes:
    """sharding.SerializeTxToBlob (sharding/collation.go:158-174) over RLP-encoded transactions (skipEvm
    false, convertTxToRawBlob); past 2^20 bytes it raises ValueError with the reference's message."""
    txs = [bytes(t) for t in encoded_txs]
    size = sum(32 * ((len(t) + 30) // 31) for t in txs)
    if size > COLLATION_SIZE_LIMIT:
        raise _size_error(size)
    return Serialize(txs, None, ctx)


def DeserializeBlobToTx(body, ctx=None):
    """sharding.DeserializeBlobToTx (sharding/collation.go:193-206), up to the RLP decode: the encoded
    transactions of a body."""
    return [b for b, _ in Deserialize(body, ctx)]


def CreateCollations(tx_lists, shard_ids, periods, proposers, keys, ctx=None):
    """proposer.createCollation over a batch (sharding/proposer/proposer.go:55-92), one prepared GPU call:
    tx_lists[i] = collation i's RLP-encoded transactions, shard_ids / periods ints, proposers 20-byte
    addresses, keys the signers' secret keys (int or up to 32 big-endian bytes; account and signer are
    separate in the reference, so the address is not derived from the key).  Returns [Collation] with the
    body serialized, the chunk root set and the header signed over its hash with ProposerSignature empty.
    A key that is no valid secret key raises crypto.ErrInvalidKey, a body past 2^20 bytes a ValueError
    with SerializeTxToBlob's message; in both cases nothing is returned.  Not done here: the SMC checks of
    createCollation (shard count, checkHeaderAdded) and AddHeader."""
    from . import crypto
    tx_lists = [[bytes(t) for t in lst] for lst in tx_lists]
    n = len(tx_lists)
    keys = [crypto._padded_key(k) for k in keys]
    if not (len(shard_ids) == len(periods) == len(proposers) == len(keys) == n):
        raise ValueError("batch sizes differ")
    if n == 0:
        return []
    for p in proposers:
        if len(bytes(p)) != 20:
            raise ValueError("a proposer address is 20 bytes")
    sid = np.frombuffer(b"".join(_int32(x) for x in shard_ids), np.uint8).reshape(n, 32)
    per = np.frombuffer(b"".join(_int32(x) for x in periods), np.uint8).reshape(n, 32)
    prop = np.frombuffer(b"".join(bytes(p) for p in proposers), np.uint8).reshape(n, 20)
    key = np.frombuffer(b"".join(keys), np.uint8).reshape(n, 32)
    bodies, root, _, sig, st = (ctx or default_context()).proposer_create_collations(tx_lists, sid, per, prop, key)
    for i in np.flatnonzero(st == _lib.ST_BODY_TOO_LARGE):
        raise _size_error(sum(32 * ((len(t) + 30) // 31) for t in tx_lists[int(i)]))
    if (st != _lib.ST_OK).any():
        raise crypto.ErrInvalidKey("invalid private key (collation %d)" % int(np.flatnonzero(st != _lib.ST_OK)[0]))
    return [Collation(CollationHeader(shard_ids[i], bytes(root[i]), periods[i], bytes(proposers[i]), bytes(sig[i])),
                      bodies[i], list(tx_lists[i])) for i in range(n)]


__all__ = ["DeriveSha", "DeriveShaBatch", "CollationHeader", "Collation", "HeaderHashBatch",
           "VerifyProposerSignatures", "CalculatePOCBatch", "ErrProposerMismatch", "COLLATION_SIZE_LIMIT",
           "Serialize", "Deserialize", "SerializeTxToBlob", "DeserializeBlobToTx", "CreateCollations", "_lib"]
