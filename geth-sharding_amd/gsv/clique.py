"""Mirror of the host half of the reference's consensus/clique package (include/gsv.h, "clique").

    Snapshot, Snapshot.apply     consensus/clique/snapshot.go; verifySeal, clique.go:478-502
    CalcDifficulty               clique.go:669-676
    the error names              clique.go:74-133

The snapshot is folded on the host (csrc/clique_host.h), in the order of the chain, over one record per header: its
hash, recovered signer, beneficiary, vote and static status (include/gsv.h gives the layout).  The library has no
batched form of the per-header half (sigHash, the static rules) yet.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib, _np_u8, _ptr
from ._lib import check
from .ethash import ErrBadHeaderRLP, ErrForkHash, ErrFutureBlock, ErrHeaderTooWide, ErrUnknownAncestor
from .params import CliqueConfig

epochLength = 30000  # clique.go:55
blockPeriod = 15     # clique.go:56
extraVanity = 32     # clique.go:58
extraSeal = 65       # clique.go:59
diffInTurn = 2       # clique.go:66
diffNoTurn = 1       # clique.go:67


class ErrInvalidCheckpointBeneficiary(ValueError):
    """errInvalidCheckpointBeneficiary (clique.go:81)"""


class ErrInvalidVote(ValueError):
    """errInvalidVote (clique.go:85)"""


class ErrInvalidCheckpointVote(ValueError):
    """errInvalidCheckpointVote (clique.go:89)"""


class ErrMissingVanity(ValueError):
    """errMissingVanity (clique.go:93)"""


class ErrMissingSignature(ValueError):
    """errMissingSignature (clique.go:97)"""


class ErrExtraSigners(ValueError):
    """errExtraSigners (clique.go:101)"""


class ErrInvalidCheckpointSigners(ValueError):
    """errInvalidCheckpointSigners (clique.go:106)"""


class ErrInvalidMixDigest(ValueError):
    """errInvalidMixDigest (clique.go:109)"""


class ErrInvalidUncleHash(ValueError):
    """errInvalidUncleHash (clique.go:112)"""


class ErrInvalidDifficulty(ValueError):
    """errInvalidDifficulty (clique.go:116)"""


class ErrInvalidTimestamp(ValueError):
    """ErrInvalidTimestamp (clique.go:120)"""


class ErrInvalidVotingChain(ValueError):
    """errInvalidVotingChain (clique.go:124)"""


class ErrUnauthorized(ValueError):
    """errUnauthorized (clique.go:127)"""


class ErrInvalidRecoveryID(ValueError):
    """secp256k1.ErrInvalidRecoveryID (secp256.go:57)"""


class ErrRecoverFailed(ValueError):
    """secp256k1.ErrRecoverFailed (secp256.go:61)"""


class ErrInvalidKey(ValueError):
    """secp256k1.ErrInvalidKey (secp256.go:58)"""


ERRORS = {
    _lib.ST_BAD_RLP: ErrBadHeaderRLP, _lib.ST_HEADER_TOO_WIDE: ErrHeaderTooWide,
    _lib.ST_UNKNOWN_ANCESTOR: ErrUnknownAncestor, _lib.ST_FUTURE_BLOCK: ErrFutureBlock, _lib.ST_FORK_HASH: ErrForkHash,
    _lib.ST_INVALID_RECID: ErrInvalidRecoveryID, _lib.ST_RECOVER_FAILED: ErrRecoverFailed,
    _lib.ST_INVALID_KEY: ErrInvalidKey,
    _lib.ST_CLIQUE_CHECKPOINT_BENEFICIARY: ErrInvalidCheckpointBeneficiary, _lib.ST_CLIQUE_INVALID_VOTE: ErrInvalidVote,
    _lib.ST_CLIQUE_CHECKPOINT_VOTE: ErrInvalidCheckpointVote, _lib.ST_CLIQUE_MISSING_VANITY: ErrMissingVanity,
    _lib.ST_CLIQUE_MISSING_SIGNATURE: ErrMissingSignature, _lib.ST_CLIQUE_EXTRA_SIGNERS: ErrExtraSigners,
    _lib.ST_CLIQUE_CHECKPOINT_SIGNERS: ErrInvalidCheckpointSigners, _lib.ST_CLIQUE_MIX_DIGEST: ErrInvalidMixDigest,
    _lib.ST_CLIQUE_UNCLE_HASH: ErrInvalidUncleHash, _lib.ST_CLIQUE_DIFFICULTY: ErrInvalidDifficulty,
    _lib.ST_CLIQUE_INVALID_TIMESTAMP: ErrInvalidTimestamp, _lib.ST_CLIQUE_UNAUTHORIZED: ErrUnauthorized,
    _lib.ST_CLIQUE_VOTING_CHAIN: ErrInvalidVotingChain}


def _raise(st: int):
    if st != _lib.ST_OK:
        raise ERRORS[st](_lib.STATUS_STRINGS[st])


def _epoch(config) -> int:
    return int(config.Epoch) or epochLength


class Snapshot:
    """The state of the authorization voting at a block (snapshot.go:46-57): an opaque gsv_clique_snapshot on the
    host.  Signers, Recents, Votes and Tally read it out; apply() folds records over it.  The object owns the C
    snapshot and frees it when it is collected: `handle` is valid only while the Snapshot itself is referenced, so
    never take the handle of a temporary (`snap.copy().handle` dangles at once)."""

    def __init__(self, signers=(), number: int = 0, hash: bytes = bytes(32), _handle=None):
        L = _lib.load()
        if _handle is None:
            rows = np.frombuffer(b"".join(bytes(s) for s in signers), np.uint8)
            if rows.size % 20:
                raise ValueError("clique: signers are 20 bytes each")
            hsh = _np_u8(bytes(hash))
            if hsh.size != 32:
                raise ValueError("clique: the hash is 32 bytes")
            _handle = L.gsv_clique_snapshot_new(_ptr(rows), rows.size // 20, int(number), _ptr(hsh))
            if not _handle:
                raise MemoryError("clique: no snapshot")
        self._h = ctypes.c_void_p(_handle)

    @classmethod
    def from_genesis(cls, header_rlp: bytes) -> "Snapshot":
        """the snapshot at block 0 with the signers of the genesis header's Extra[32 : len - 65] (clique.go:392-401)"""
        blob = _np_u8(bytes(header_rlp))
        st = ctypes.c_int(0)
        h = _lib.load().gsv_clique_snapshot_from_genesis(_ptr(blob), blob.size, ctypes.byref(st))
        if not h:
            _raise(st.value or _lib.ST_BAD_RLP)
        return cls(_handle=h)

    def copy(self) -> "Snapshot":
        h = _lib.load().gsv_clique_snapshot_copy(self._h)
        if not h:
            raise MemoryError("clique: no snapshot")
        return Snapshot(_handle=h)

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().gsv_clique_snapshot_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    @property
    def Number(self) -> int:
        return int(_lib.load().gsv_clique_snapshot_number(self._h))

    @property
    def Hash(self) -> bytes:
        out = np.zeros(32, np.uint8)
        check(_lib.load().gsv_clique_snapshot_hash(self._h, _ptr(out)))
        return out.tobytes()

    def signers(self):
        """the authorized signers in ascending order (snapshot.go:288-301)"""
        L = _lib.load()
        n = int(L.gsv_clique_snapshot_signers(self._h, None, 0))
        out = np.zeros((max(n, 1), 20), np.uint8)
        L.gsv_clique_snapshot_signers(self._h, _ptr(out), n)
        return [out[i].tobytes() for i in range(n)]

    @property
    def Signers(self):
        return set(self.signers())

    @property
    def Recents(self):
        """{block: signer}"""
        L = _lib.load()
        n = int(L.gsv_clique_snapshot_recents(self._h, None, None, 0))
        blk, sg = np.zeros(max(n, 1), np.uint64), np.zeros((max(n, 1), 20), np.uint8)
        L.gsv_clique_snapshot_recents(self._h, _ptr(blk), _ptr(sg), n)
        return {int(blk[i]): sg[i].tobytes() for i in range(n)}

    @property
    def Votes(self):
        """[(signer, block, address, authorize)] in chronological order"""
        L = _lib.load()
        n = int(L.gsv_clique_snapshot_votes(self._h, None, None, None, None, 0))
        sg, blk = np.zeros((max(n, 1), 20), np.uint8), np.zeros(max(n, 1), np.uint64)
        ad, au = np.zeros((max(n, 1), 20), np.uint8), np.zeros(max(n, 1), np.uint8)
        L.gsv_clique_snapshot_votes(self._h, _ptr(sg), _ptr(blk), _ptr(ad), _ptr(au), n)
        return [(sg[i].tobytes(), int(blk[i]), ad[i].tobytes(), bool(au[i])) for i in range(n)]

    @property
    def Tally(self):
        """{address: (authorize, votes)}"""
        L = _lib.load()
        n = int(L.gsv_clique_snapshot_tally(self._h, None, None, None, 0))
        ad, au = np.zeros((max(n, 1), 20), np.uint8), np.zeros(max(n, 1), np.uint8)
        vt = np.zeros(max(n, 1), np.int32)
        L.gsv_clique_snapshot_tally(self._h, _ptr(ad), _ptr(au), _ptr(vt), n)
        return {ad[i].tobytes(): (bool(au[i]), int(vt[i])) for i in range(n)}

    def inturn(self, number: int, signer: bytes) -> bool:
        """Snapshot.inturn (snapshot.go:304-310)"""
        sg = _np_u8(bytes(signer))
        return bool(_lib.load().gsv_clique_snapshot_inturn(self._h, int(number), _ptr(sg)))

    def apply(self, config, records, headers):
        """gsv_clique_fold: verifySeal and Snapshot.apply over the records (n x 128 bytes) of consecutive headers,
        `headers` their RLP.  Moves this snapshot to the last header applied; returns (status (n,), applied)."""
        rec = np.ascontiguousarray(records, np.uint8).reshape(-1, _lib.CLIQUE_RECORD_BYTES)
        headers = [bytes(h) for h in headers]
        n = rec.shape[0]
        if len(headers) != n:
            raise ValueError("clique: one record per header")
        lens = np.fromiter((len(h) for h in headers), dtype=np.uint64, count=n)
        off = np.zeros(n + 1, np.uint64)
        np.cumsum(lens, out=off[1:])
        flat = np.frombuffer(b"".join(headers) + b"\0" * 8, np.uint8)
        st = np.zeros(n, np.uint8)
        applied = ctypes.c_size_t(0)
        cfg = _lib.CliqueConfigStruct(int(config.Period), _epoch(config))
        check(_lib.load().gsv_clique_fold(self._h, ctypes.byref(cfg), _ptr(rec), n, _ptr(flat), _ptr(off), _ptr(st),
                                          ctypes.byref(applied)))
        return st, int(applied.value)


def CalcDifficulty(snap: Snapshot, signer: bytes) -> int:
    """CalcDifficulty(snap, signer) (clique.go:669-676): 2 when the signer is in turn at snap.Number + 1, else 1"""
    sg = _np_u8(bytes(signer))
    return int(_lib.load().gsv_clique_calc_difficulty(snap.handle, _ptr(sg)))


__all__ = ["Snapshot", "CalcDifficulty", "CliqueConfig", "ERRORS"] + \
    [k for k in list(globals()) if k.startswith("Err")]
