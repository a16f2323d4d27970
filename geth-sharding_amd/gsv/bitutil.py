"""common/bitutil's sparse bitset codec (compress.go) over batches, on the GPU.

    CompressBytes / DecompressBytes     common/bitutil/compress.go:60-67, :102-112

A vector is at most _lib.BITSET_MAX_LEN bytes (ours; a bloombits vector of the largest section is 4,096).  The
batch forms take vectors of one length, as the bit vectors of a section are.
"""
from __future__ import annotations

import numpy as np

from . import _lib, default_context


class BitsetError(ValueError):
    """a decompression error of compress.go:21-37 (`status`: the GSV_ST_BITSET_* code)"""
    status = 0

    def __init__(self):
        super().__init__(_lib.STATUS_STRINGS[self.status])


class ErrMissingData(BitsetError):
    status = _lib.ST_BITSET_MISSING_DATA


class ErrUnreferencedData(BitsetError):
    status = _lib.ST_BITSET_UNREFERENCED_DATA


class ErrExceededTarget(BitsetError):
    status = _lib.ST_BITSET_EXCEEDED_TARGET


class ErrZeroContent(BitsetError):
    status = _lib.ST_BITSET_ZERO_CONTENT


ERRORS = {e.status: e for e in (ErrMissingData, ErrUnreferencedData, ErrExceededTarget, ErrZeroContent)}


def _check_len(n: int):
    if n > _lib.BITSET_MAX_LEN:
        raise ValueError(f"bitutil: a vector of {n} bytes is above GSV_BITSET_MAX_LEN ({_lib.BITSET_MAX_LEN})")


def CompressBytesBatch(vectors, ctx=None):
    """CompressBytes of each of n vectors of one length: a list of bytes"""
    vectors = [bytes(v) for v in vectors]
    if not vectors:
        return []
    length = len(vectors[0])
    if any(len(v) != length for v in vectors):
        raise ValueError("bitutil: the vectors of a batch have one length")
    _check_len(length)
    if length == 0:  # compress.go:73-75: nil is not shorter than nothing, the copy is empty
        return [b""] * len(vectors)
    rows = np.frombuffer(b"".join(vectors), np.uint8).reshape(len(vectors), length)
    return (ctx or default_context()).bitset_compress_batch(rows)


def CompressBytes(data, ctx=None) -> bytes:
    return CompressBytesBatch([data], ctx)[0]


def DecompressBytesBatch(items, target: int, ctx=None):
    """DecompressBytes(item, target) of each byte string: (rows (n, target) uint8, status (n,) uint8); a failed
    item's row is zero and its status the GSV_ST_BITSET_* code of the reference's error"""
    items = [bytes(x) for x in items]
    target = int(target)
    if target < 0:
        raise ValueError("bitutil: a negative target")
    _check_len(target)
    if target == 0:  # compress.go:103-105, :132-134: answered here, nothing to launch
        st = np.array([_lib.ST_BITSET_EXCEEDED_TARGET if x else _lib.ST_OK for x in items], np.uint8)
        return np.zeros((len(items), 0), np.uint8), st
    return (ctx or default_context()).bitset_decompress_batch(items, target)


def DecompressBytes(data, target: int, ctx=None) -> bytes:
    rows, st = DecompressBytesBatch([data], target, ctx)
    if st[0]:
        raise ERRORS[int(st[0])]()
    return rows[0].tobytes()
