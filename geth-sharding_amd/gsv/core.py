"""Mirror of the reference's core package where it validates a block against its receipts, batched on the GPU.

    ValidateReceipts(lists, blooms, receipt_hashes, gas_used)    the receipt half of
                                 BlockValidator.ValidateState (core/block_validator.go:80-95)

Receipts travel as their consensus RLP (Receipts.GetRlp(i), core/types/receipt.go:98-100), one list per block.
"""
from __future__ import annotations

from . import _lib, default_context


class ErrGasUsedMismatch(ValueError):
    """invalid gas used (block_validator.go:82-84)"""


class ErrInvalidBloom(ValueError):
    """invalid bloom (block_validator.go:87-90)"""


class ErrInvalidReceiptRoot(ValueError):
    """invalid receipt root hash (block_validator.go:92-95)"""


ERRORS = {_lib.ST_GAS_USED_MISMATCH: ErrGasUsedMismatch, _lib.ST_INVALID_BLOOM: ErrInvalidBloom,
          _lib.ST_INVALID_RECEIPT_ROOT: ErrInvalidReceiptRoot}


def ValidateReceipts(lists, blooms=None, receipt_hashes=None, gas_used=None, ctx=None):
    """The RECEIPT half of BlockValidator.ValidateState (core/block_validator.go:80-95) for a batch of blocks:
    per block, the gas used against the header's (:82-84), the bloom of its receipts against header.Bloom
    (:87-90) and DeriveSha(receipts) against header.ReceiptHash (:92-95), in that order.  The other half, the
    state root (IntermediateRoot against header.Root, :98-100), needs the state database and STAYS WITH THE
    CALLER: a block that passes here is not yet valid.

    lists[i]: block i's receipts as their consensus RLP.  blooms (n x 256 bytes), receipt_hashes (n x 32 bytes),
    gas_used (n integers): the headers' values; each None skips that compare, so with all three None this is
    CreateBloom and the receipt root.  Returns (status (n,) uint8, blooms (n, 256), roots (n, 32), gas used (n,)
    uint64).  status: ST_OK, ST_GAS_USED_MISMATCH, ST_INVALID_BLOOM, ST_INVALID_RECEIPT_ROOT, or, OURS, the
    ST_BAD_RLP / ST_RECEIPT_STATUS of the block's first receipt that does not decode (zero rows, gas 0)."""
    st, _, bloom, root, gas = (ctx or default_context()).receipts_verify_batch(lists, blooms, receipt_hashes, gas_used)
    return st, bloom, root, gas


__all__ = ["ValidateReceipts", "ErrGasUsedMismatch", "ErrInvalidBloom", "ErrInvalidReceiptRoot", "ERRORS"]
