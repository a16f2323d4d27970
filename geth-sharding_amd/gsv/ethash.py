"""Mirror of the reference's consensus/ethash: the seal check of a light verifier and the sealer's search,
batched on the GPU.

    cacheSize(block), datasetSize(block)   algorithm.go:53-91 (the formula; the tables hold its values)
    seedHash(block)                        algorithm.go:110-120
    generateCache(size, seed)              algorithm.go:128-197, on the host (include/gsv.h says why)
    generateDatasetItems(cache, first, count)   generateDatasetItem over a range: the body of generateDataset
    generateDataset(size, cache)                algorithm.go:265-328 -> the dataset as a device tensor
    hashimotoLight(size, cache, hash, nonce)    algorithm.go:375 -> (digest, result)
    hashimotoLightBatch(size, cache, hashes, nonces)
    hashimotoFull(dataset, hash, nonce)         algorithm.go:393-405 -> (digest, result)
    hashimotoFullBatch(dataset, hashes, nonces)
    Ethash(test_mode).VerifySeal / VerifySeals  consensus.go:463-501, by block number
    Ethash(test_mode).hashimotoFull             by block number, over the context's epoch datasets
    Ethash(test_mode).Seal / SealBatch          the search of mine (sealer.go:97-152), by block number

    CalcDifficulty(config, time, parent_rlp)    consensus.go:297-459 over an RLP-encoded parent
    Ethash(test_mode).VerifyHeaders / VerifyHeader   consensus.go:90-166, :223-285 over RLP-encoded headers

The nonce is the number (Header.Nonce.Uint64()); types.BlockNonce is its big-endian bytes.  Not here: VerifyUncles,
the known-block lookup of verifyHeaderWorker (the caller's database), Prepare / Finalize, DAG and cache files on
disk, remote mining / GetWork, and pre-generating the next epoch.
"""
from __future__ import annotations

import numpy as np

from . import _lib, _np_u8, _ptr, _rows32, default_context
from ._lib import check

epochLength = 30000
MAX_UINT256 = (1 << 256) - 1


class ErrInvalidDifficulty(ValueError):
    """errInvalidDifficulty (consensus.go:56)"""


class ErrInvalidMixDigest(ValueError):
    """errInvalidMixDigest (consensus.go:57)"""


class ErrInvalidPoW(ValueError):
    """errInvalidPoW (consensus.go:58)"""


_ERRORS = {_lib.ST_INVALID_DIFFICULTY: ErrInvalidDifficulty, _lib.ST_INVALID_MIX_DIGEST: ErrInvalidMixDigest,
           _lib.ST_INVALID_POW: ErrInvalidPoW}


class ErrBadHeaderRLP(ValueError):
    """rlp: the header does not decode"""


class ErrHeaderTooWide(ValueError):
    """Difficulty or Time above 32 bytes, or Number above 8 (this library's bound, not the reference's)"""


class ErrUnknownAncestor(ValueError):
    """consensus.ErrUnknownAncestor (consensus/errors.go:24)"""


class ErrExtraTooLong(ValueError):
    """"extra-data too long" (consensus.go:225-227)"""


class ErrFutureBlock(ValueError):
    """consensus.ErrFutureBlock (consensus/errors.go:32)"""


class ErrZeroBlockTime(ValueError):
    """errZeroBlockTime (consensus.go:51)"""


class ErrWrongDifficulty(ValueError):
    """"invalid difficulty: have .., want .." (consensus.go:244-246)"""


class ErrGasLimitCap(ValueError):
    """"invalid gasLimit: have .., max .." (consensus.go:248-251)"""


class ErrGasUsed(ValueError):
    """"invalid gasUsed: have .., gasLimit .." (consensus.go:253-255)"""


class ErrGasLimitBounds(ValueError):
    """"invalid gas limit: have .., want .. += .." (consensus.go:258-266)"""


class ErrInvalidNumber(ValueError):
    """consensus.ErrInvalidNumber (consensus/errors.go:36)"""


class ErrBadProDAOExtra(ValueError):
    """misc.ErrBadProDAOExtra (consensus/misc/dao.go:32)"""


class ErrBadNoDAOExtra(ValueError):
    """misc.ErrBadNoDAOExtra (consensus/misc/dao.go:36)"""


class ErrForkHash(ValueError):
    """"homestead gas reprice fork: have .., want .." (consensus/misc/forks.go:36-39)"""


_HEADER_ERRORS = dict(_ERRORS)
_HEADER_ERRORS.update({
    _lib.ST_BAD_RLP: ErrBadHeaderRLP, _lib.ST_HEADER_TOO_WIDE: ErrHeaderTooWide,
    _lib.ST_UNKNOWN_ANCESTOR: ErrUnknownAncestor, _lib.ST_EXTRA_TOO_LONG: ErrExtraTooLong,
    _lib.ST_FUTURE_BLOCK: ErrFutureBlock, _lib.ST_ZERO_BLOCK_TIME: ErrZeroBlockTime,
    _lib.ST_WRONG_DIFFICULTY: ErrWrongDifficulty, _lib.ST_GAS_LIMIT_CAP: ErrGasLimitCap, _lib.ST_GAS_USED: ErrGasUsed,
    _lib.ST_GAS_LIMIT_BOUNDS: ErrGasLimitBounds, _lib.ST_INVALID_NUMBER: ErrInvalidNumber,
    _lib.ST_BAD_PRO_DAO_EXTRA: ErrBadProDAOExtra, _lib.ST_BAD_NO_DAO_EXTRA: ErrBadNoDAOExtra,
    _lib.ST_FORK_HASH: ErrForkHash})


def CalcDifficultyBatch(config, times, parent_rlps, ctx=None):
    """(difficulties: list of int, status (n,)): CalcDifficulty(config, times[i], parent i) over RLP-encoded
    parents.  A parent that does not decode has its decode status and difficulty None; a value of 2^256 or more
    has ST_WRONG_DIFFICULTY and difficulty None."""
    rows, st = (ctx or default_context()).calc_difficulty_batch(config, times, parent_rlps)
    return [int.from_bytes(r.tobytes(), "big") if s == _lib.ST_OK else None for r, s in zip(rows, st)], st


def CalcDifficulty(config, time: int, parent_rlp: bytes, ctx=None) -> int:
    """CalcDifficulty(config, time, parent) (consensus.go:297-459), the parent as its RLP encoding.  Raises
    ErrBadHeaderRLP / ErrHeaderTooWide for the parent, OverflowError for a value of 2^256 or more."""
    vals, st = CalcDifficultyBatch(config, [int(time)], [parent_rlp], ctx)
    if st[0] == _lib.ST_WRONG_DIFFICULTY:
        raise OverflowError("ethash: the difficulty is 2^256 or more")
    if st[0] != _lib.ST_OK:
        raise _HEADER_ERRORS[int(st[0])](_lib.STATUS_STRINGS[int(st[0])])
    return vals[0]


def cacheSize(block: int) -> int:
    return int(_lib.load().gsv_ethash_cache_size(int(block)))


def datasetSize(block: int) -> int:
    return int(_lib.load().gsv_ethash_dataset_size(int(block)))


def seedHash(block: int) -> bytes:
    out = np.zeros(32, np.uint8)
    check(_lib.load().gsv_ethash_seed_hash(int(block), _ptr(out)))
    return out.tobytes()


def generateCache(size: int, seed: bytes) -> np.ndarray:
    """the verification cache of `size` bytes for `seed`, as uint8 (the reference's words, little-endian)"""
    seed = _np_u8(seed)
    if seed.shape != (32,):
        raise ValueError("ethash: the seed is 32 bytes")
    out = np.zeros(int(size), np.uint8)
    check(_lib.load().gsv_ethash_make_cache(_ptr(seed), int(size), _ptr(out)))
    return out


def _device_cache(cache, ctx):
    """the cache as a CUDA uint8 tensor on the context's device (a tensor already there is used as it is)"""
    import torch
    if isinstance(cache, torch.Tensor):
        return cache
    return torch.from_numpy(np.ascontiguousarray(_np_u8(cache))).to(f"cuda:{ctx.device}")


def generateDatasetItems(cache, first: int, count: int, ctx=None) -> np.ndarray:
    """dataset items [first, first + count) as (count, 64) uint8"""
    import torch
    ctx = ctx or default_context()
    d_cache = _device_cache(cache, ctx)
    out = torch.empty((int(count), 64), dtype=torch.uint8, device=d_cache.device)
    ctx.ethash_dataset_items_dev(d_cache, first, count, out)
    torch.cuda.synchronize(d_cache.device)
    return out.cpu().numpy()


def hashimotoLightBatch(size: int, cache, hashes, nonces, ctx=None):
    """(digests (n, 32), results (n, 32)) of hashimotoLight(size, cache, hashes[i], nonces[i])"""
    import torch
    ctx = ctx or default_context()
    d_cache = _device_cache(cache, ctx)
    h = _rows32(hashes)
    nn = np.ascontiguousarray(nonces, np.uint64).reshape(-1)
    n = h.shape[0]
    if nn.shape[0] != n:
        raise ValueError("ethash: one 32-byte hash and one nonce per item")
    dev = d_cache.device
    d_h = torch.from_numpy(h).to(dev)
    d_n = torch.from_numpy(nn.view(np.int64)).to(dev)
    d_mix = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    d_res = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    ctx.ethash_light_batch_dev(d_cache, size, d_h, d_n, d_mix, d_res, n=n)
    torch.cuda.synchronize(dev)
    return d_mix.cpu().numpy(), d_res.cpu().numpy()


def hashimotoLight(size: int, cache, hash: bytes, nonce: int, ctx=None):
    mix, res = hashimotoLightBatch(size, cache, [bytes(hash)], [int(nonce)], ctx)
    return mix[0].tobytes(), res[0].tobytes()


def generateDataset(size: int, cache, ctx=None):
    """the dataset of `size` bytes (a multiple of 128) over `cache`, generated on the device: a CUDA uint8
    tensor of `size` bytes, which hashimotoFull and Context.ethash_search_dev read in place"""
    import torch
    size = int(size)
    if size < 128 or size % 128:
        raise ValueError("ethash: the dataset size is a multiple of 128 bytes")
    ctx = ctx or default_context()
    d_cache = _device_cache(cache, ctx)
    out = torch.empty(size, dtype=torch.uint8, device=d_cache.device)
    items, step = size // 64, 1 << 31
    for first in range(0, items, step):
        count = min(step, items - first)
        ctx.ethash_dataset_items_dev(d_cache, first, count, out[first * 64:(first + count) * 64])
    torch.cuda.synchronize(d_cache.device)
    return out


def hashimotoFullBatch(dataset, hashes, nonces, ctx=None):
    """(digests (n, 32), results (n, 32)) of hashimotoFull(dataset, hashes[i], nonces[i]); dataset is
    generateDataset's tensor (or the dataset's bytes on the host, uploaded here)"""
    import torch
    ctx = ctx or default_context()
    d_set = _device_cache(dataset, ctx)
    h = _rows32(hashes)
    nn = np.ascontiguousarray(nonces, np.uint64).reshape(-1)
    n = h.shape[0]
    if nn.shape[0] != n:
        raise ValueError("ethash: one 32-byte hash and one nonce per item")
    dev = d_set.device
    d_h = torch.from_numpy(h).to(dev)
    d_n = torch.from_numpy(nn.view(np.int64)).to(dev)
    d_mix = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    d_res = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    ctx.ethash_full_batch_dev(d_set, d_h, d_n, d_mix, d_res, n=n)
    torch.cuda.synchronize(dev)
    return d_mix.cpu().numpy(), d_res.cpu().numpy()


def hashimotoFull(dataset, hash: bytes, nonce: int, ctx=None):
    mix, res = hashimotoFullBatch(dataset, [bytes(hash)], [int(nonce)], ctx)
    return mix[0].tobytes(), res[0].tobytes()


def _difficulty_rows(difficulties) -> np.ndarray:
    """32 bytes big-endian per difficulty.  Negative means non-positive (row of zeros: ErrInvalidDifficulty);
    2^256 and more cannot be written in 32 bytes and is handled by the caller."""
    rows = np.zeros((len(difficulties), 32), np.uint8)
    for i, d in enumerate(difficulties):
        d = int(d)
        if 0 < d <= MAX_UINT256:
            rows[i] = np.frombuffer(d.to_bytes(32, "big"), np.uint8)
    return rows


class Ethash:
    """consensus.Engine's seal check.  test_mode is the reference's ModeTest: a 1,024-byte cache, still seeded
    by the epoch, and a 32 KiB dataset."""

    def __init__(self, test_mode: bool = False, ctx=None):
        self.test_mode = bool(test_mode)
        self.ctx = ctx or default_context()

    def hashimotoLight(self, numbers, hashes, nonces):
        return self.ctx.ethash_light_batch(numbers, hashes, nonces, self.test_mode)

    def VerifySeals(self, numbers, hashes_no_nonce, nonces, mix_digests, difficulties) -> np.ndarray:
        """status (n,) uint8 per header: ST_OK, ST_INVALID_DIFFICULTY, ST_INVALID_MIX_DIGEST or ST_INVALID_POW.
        difficulties: Python ints, or (n, 32) big-endian rows."""
        if isinstance(difficulties, np.ndarray) and difficulties.dtype == np.uint8:
            return self.ctx.ethash_verify_seal_batch(numbers, hashes_no_nonce, nonces, mix_digests, difficulties,
                                                     self.test_mode)
        difficulties = [int(d) for d in difficulties]
        # A difficulty of 2^256 or more has target floor((2^256 - 1) / d) = 0: only a zero result passes.  The
        # library sees it as difficulty 2^256 - 1 (target 1: mix and difficulty checks as ever), and a result
        # of exactly one is failed here.
        big = [i for i, d in enumerate(difficulties) if d > MAX_UINT256]
        rows = _difficulty_rows([MAX_UINT256 if d > MAX_UINT256 else d for d in difficulties])
        st = self.ctx.ethash_verify_seal_batch(numbers, hashes_no_nonce, nonces, mix_digests, rows, self.test_mode)
        ok_big = [i for i in big if st[i] == _lib.ST_OK]
        if ok_big:
            num = np.ascontiguousarray(numbers, np.uint64).reshape(-1)[ok_big]
            h = _rows32(hashes_no_nonce)[ok_big]
            nn = np.ascontiguousarray(nonces, np.uint64).reshape(-1)[ok_big]
            _, res = self.ctx.ethash_light_batch(num, h, nn, self.test_mode)
            for k, i in enumerate(ok_big):
                if res[k].any():
                    st[i] = _lib.ST_INVALID_POW
        return st

    def hashimotoFull(self, numbers, hashes, nonces):
        """as hashimotoLight, over the epochs' datasets (generated on the device, at most
        _lib.ETHASH_MAX_DATASETS kept by the context)"""
        return self.ctx.ethash_full_batch(numbers, hashes, nonces, self.test_mode)

    def SealBatch(self, numbers, hashes_no_nonce, difficulties, start_nonces, max_attempts: int):
        """The sealer's search per header: (nonces (n,) uint64, mix digests (n, 32), status (n,) uint8: ST_OK,
        ST_INVALID_DIFFICULTY or ST_NONCE_NOT_FOUND).  Header i tries start_nonces[i], start_nonces[i] + 1, ...
        (mod 2^64) for at most max_attempts nonces and reports the FIRST whose result is within the target:
        what mine() finds from that seed as the only thread.  difficulties: Python ints, or (n, 32) big-endian
        rows."""
        max_attempts = int(max_attempts)
        if isinstance(difficulties, np.ndarray) and difficulties.dtype == np.uint8:
            return self.ctx.ethash_seal_batch(numbers, hashes_no_nonce, difficulties, start_nonces, max_attempts,
                                              self.test_mode)
        difficulties = [int(d) for d in difficulties]
        # 2^256 and more: target 0, only a zero result seals.  As in VerifySeals the library sees 2^256 - 1
        # (target 1); a winner whose result is one is passed over here and the search goes on behind it.
        big = [i for i, d in enumerate(difficulties) if d > MAX_UINT256]
        rows = _difficulty_rows([MAX_UINT256 if d > MAX_UINT256 else d for d in difficulties])
        nonce, mix, st = self.ctx.ethash_seal_batch(numbers, hashes_no_nonce, rows, start_nonces, max_attempts,
                                                    self.test_mode)
        if big:
            num = np.ascontiguousarray(numbers, np.uint64).reshape(-1)
            h = _rows32(hashes_no_nonce)
            first = np.ascontiguousarray(start_nonces, np.uint64).reshape(-1)
            for i in big:
                while st[i] == _lib.ST_OK:
                    _, res = self.ctx.ethash_full_batch(num[i:i + 1], h[i:i + 1], nonce[i:i + 1], self.test_mode)
                    if not res.any():
                        break
                    used = ((int(nonce[i]) - int(first[i])) % (1 << 64)) + 1
                    nxt = np.array([(int(nonce[i]) + 1) % (1 << 64)], np.uint64)
                    n1, m1, s1 = self.ctx.ethash_seal_batch(num[i:i + 1], h[i:i + 1], rows[i:i + 1], nxt,
                                                            max_attempts - used, self.test_mode)
                    nonce[i], mix[i], st[i] = n1[0], m1[0], s1[0]
        return nonce, mix, st

    def Seal(self, number: int, hash_no_nonce: bytes, difficulty: int, start_nonce: int, max_attempts: int):
        """(nonce, mix digest) of the first seal at or after start_nonce, or None when none lies within
        max_attempts nonces.  Raises ErrInvalidDifficulty for a non-positive difficulty."""
        nonce, mix, st = self.SealBatch([number], [bytes(hash_no_nonce)], [difficulty], [start_nonce], max_attempts)
        if st[0] == _lib.ST_INVALID_DIFFICULTY:
            raise ErrInvalidDifficulty(_lib.STATUS_STRINGS[_lib.ST_INVALID_DIFFICULTY])
        if st[0] != _lib.ST_OK:
            return None
        return int(nonce[0]), mix[0].tobytes()

    def VerifyHeaders(self, config, headers, seals=None, parent=None, now=None) -> np.ndarray:
        """Ethash.VerifyHeaders (consensus.go:90-166): status (n,) uint8 per RLP-encoded header, the reference's
        errors in the reference's order (include/gsv.h lists them).  seals: one flag per header, None = all;
        parent: the RLP of header 0's parent, standing for chain.GetHeader(ParentHash, Number - 1); now: Unix
        seconds, None = the clock.  The known-block short cut of verifyHeaderWorker is the caller's database and
        is not here."""
        if now is None:
            import time
            now = int(time.time())
        return self.ctx.ethash_verify_headers_batch(config, headers, seals, parent, now, self.test_mode)

    def VerifyHeader(self, config, header: bytes, parent: bytes, seal: bool = True, now=None) -> None:
        """Ethash.VerifyHeader (consensus.go:71-84) of one RLP-encoded header against its parent: raises the
        exception class of the reference's error"""
        st = int(self.VerifyHeaders(config, [header], [seal], parent, now)[0])
        if st != _lib.ST_OK:
            raise _HEADER_ERRORS[st](_lib.STATUS_STRINGS[st])

    def VerifySeal(self, number: int, hash_no_nonce: bytes, nonce: int, mix_digest: bytes, difficulty: int) -> None:
        st = int(self.VerifySeals([number], [bytes(hash_no_nonce)], [nonce], [bytes(mix_digest)], [difficulty])[0])
        if st != _lib.ST_OK:
            raise _ERRORS[st](_lib.STATUS_STRINGS[st])
