"""gsv — MI355X-native batch validation engine for geth-sharding's collation-validation hot path.

Host-side mirror of the reference's Go APIs for this path, over the C ABI of libgsv.so
(include/gsv.h).  Every call runs the hand-written HIP kernels for gfx950; there is no CPU
fallback (a missing libgsv.so or GPU raises).

    crypto.Ecrecover / SigToPub / Keccak256      crypto/signature_cgo.go:31-44, crypto/crypto.go:43
    types.Sender + EIP155/Homestead/Frontier     core/types/transaction_signing.go:72-247
    sharding.CalculateChunkRoot / DeriveSha      sharding/collation.go:115-119, core/types/derive_sha.go:32
    bn256.PairingCheck / precompile Run          crypto/bn256/cloudflare/bn256.go:313-327, core/vm/contracts.go:333
"""
from __future__ import annotations

import atexit
import ctypes
import os
import threading
import weakref

import numpy as np

from . import _lib
from ._lib import GsvError, check

__all__ = ["Context", "default_context", "GsvError", "device_count"]


def _np_u8(a) -> np.ndarray:
    if isinstance(a, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(a), np.uint8)
    return np.ascontiguousarray(a, dtype=np.uint8)


def _ptr(a: np.ndarray):
    return ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else None


def _pack(msgs):
    """list of bytes -> (flat uint8 array, uint64 offsets[n+1])"""
    lens = np.fromiter((len(m) for m in msgs), dtype=np.uint64, count=len(msgs))
    off = np.zeros(len(msgs) + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    flat = np.frombuffer(b"".join(bytes(m) for m in msgs) + b"\0" * 8, np.uint8)
    return flat, off


def device_count() -> int:
    return int(_lib.load().gsv_device_count())


class Context:
    """One libgsv context (one HIP device): stream, HBM staging arena, precomputed tables."""

    def __init__(self, device: int = 0):
        L = _lib.load()
        h = ctypes.c_void_p()
        check(L.gsv_ctx_create(int(device), ctypes.byref(h)))
        self._h = h
        self.device = int(device)
        self._streams = []  # gsv_stream_create handles not yet destroyed
        _live.add(self)

    # -------------------------------------------------------------- lifecycle / timing
    def close(self):
        """Destroys the context and the streams it made (gsv_ctx_destroy also destroys any the caller left
        live).  Every live Context is closed at interpreter exit (atexit), before the HIP runtime's own
        static teardown, never from __del__ during module teardown."""
        if getattr(self, "_h", None):
            for q in self._streams:
                _lib.load().gsv_stream_destroy(self._h, q)
            self._streams = []
            _lib.load().gsv_ctx_destroy(self._h)
            self._h = None

    def stream_count(self):
        """(live gsv_stream_create streams, live side streams of prepared shapes)"""
        u, s = ctypes.c_int(), ctypes.c_int()
        check(_lib.load().gsv_ctx_stream_count(self._h, ctypes.byref(u), ctypes.byref(s)))
        return u.value, s.value

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def set_timing(self, on: bool):
        check(_lib.load().gsv_ctx_set_timing(self._h, 1 if on else 0))

    def kernel_time(self, kid: int):
        ms = ctypes.c_double()
        n = ctypes.c_long()
        check(_lib.load().gsv_ctx_kernel_time(self._h, kid, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def set_pipeline_depth(self, depth: int):
        """Instances per prepared shape from now on (gsv_ctx_set_pipeline_depth): *_dev calls of one
        shape on up to `depth` streams run concurrently."""
        check(_lib.load().gsv_ctx_set_pipeline_depth(self._h, int(depth)))

    def pipeline_streams(self, n: int):
        """`n` streams on hardware queues of their own (gsv_stream_create), as torch ExternalStreams: the
        streams of a pipeline of `n` batches (torch's pool streams can share an in-order queue, and
        batches on them then serialise).  At most _lib.MAX_STREAMS live per context."""
        import torch
        if len(self._streams) + int(n) > _lib.MAX_STREAMS:
            raise GsvError(f"{len(self._streams)} pipeline streams live, {n} more exceeds GSV_MAX_STREAMS "
                           f"({_lib.MAX_STREAMS}): destroy_streams() the previous pipeline's first")
        out = []
        for _ in range(int(n)):
            q = ctypes.c_void_p()
            check(_lib.load().gsv_stream_create(self._h, ctypes.byref(q)))
            self._streams.append(q.value)
            out.append(torch.cuda.ExternalStream(q.value, device=torch.device("cuda", self.device)))
        return out

    def destroy_streams(self, streams):
        """Destroys streams from pipeline_streams (after their work)."""
        for st in streams:
            q = int(st.cuda_stream)
            if q in self._streams:
                self._streams.remove(q)
                check(_lib.load().gsv_stream_destroy(self._h, q))

    def reset_timing(self):
        check(_lib.load().gsv_ctx_reset_timing(self._h))

    # -------------------------------------------------------------- Keccak-256
    def keccak256_batch(self, msgs) -> np.ndarray:
        n = len(msgs)
        out = np.zeros((n, 32), np.uint8)
        if n == 0:
            return out
        flat, off = _pack(msgs)
        check(_lib.load().gsv_keccak256_batch(self._h, _ptr(flat), _ptr(off), n, _ptr(out)))
        return out

    # -------------------------------------------------------------- SHA-256, RIPEMD-160
    def _md_batch(self, fn, msgs) -> np.ndarray:
        n = len(msgs)
        out = np.zeros((n, 32), np.uint8)
        if n == 0:
            return out
        flat, off = _pack(msgs)
        check(fn(self._h, _ptr(flat), _ptr(off), n, _ptr(out)))
        return out

    def sha256_batch(self, msgs) -> np.ndarray:
        """(n, 32) uint8: SHA-256 of each message (gsv.h gsv_sha256_batch)"""
        return self._md_batch(_lib.load().gsv_sha256_batch, msgs)

    def ripemd160_batch(self, msgs) -> np.ndarray:
        """(n, 32) uint8: the ripemd160hash precompile's row of each message, 12 zero bytes and the 20-byte
        RIPEMD-160 digest (gsv.h gsv_ripemd160_batch)"""
        return self._md_batch(_lib.load().gsv_ripemd160_batch, msgs)

    # -------------------------------------------------------------- secp256k1
    def ecrecover_batch(self, msg32, sig65, want_pub=True, want_addr=False):
        """msg32 (n,32) uint8, sig65 (n,65) uint8 -> (pub65 (n,65) | None, addr20 (n,20) | None,
        status (n,))  with ext.h / secp256.go semantics per item."""
        msg32 = np.ascontiguousarray(msg32, np.uint8).reshape(-1, 32)
        sig65 = np.ascontiguousarray(sig65, np.uint8).reshape(-1, 65)
        n = msg32.shape[0]
        if sig65.shape[0] != n:
            raise ValueError("msg32 and sig65 batch sizes differ")
        pub = np.zeros((n, 65), np.uint8) if want_pub else None
        addr = np.zeros((n, 20), np.uint8) if want_addr else None
        st = np.zeros(n, np.uint8)
        if n:
            check(_lib.load().gsv_ecrecover_batch(self._h, _ptr(msg32), _ptr(sig65), n, _ptr(pub),
                                                  _ptr(addr), _ptr(st)))
        return pub, addr, st

    def sender_batch(self, sighash32, r32, s32, v, v_big, homestead: bool):
        sighash32 = np.ascontiguousarray(sighash32, np.uint8).reshape(-1, 32)
        n = sighash32.shape[0]
        r32 = np.ascontiguousarray(r32, np.uint8).reshape(n, 32)
        s32 = np.ascontiguousarray(s32, np.uint8).reshape(n, 32)
        v = np.ascontiguousarray(v, np.uint64).reshape(n)
        v_big = np.ascontiguousarray(v_big, np.uint8).reshape(n)
        addr = np.zeros((n, 20), np.uint8)
        st = np.zeros(n, np.uint8)
        if n:
            check(_lib.load().gsv_sender_batch(self._h, _ptr(sighash32), _ptr(r32), _ptr(s32), _ptr(v),
                                               _ptr(v_big), n, 1 if homestead else 0, _ptr(addr),
                                               _ptr(st)))
        return addr, st

    def tx_sender_batch(self, txs, chain_id: int, signer_kind: int):
        n = len(txs)
        addr = np.zeros((n, 20), np.uint8)
        st = np.zeros(n, np.uint8)
        if n == 0:
            return addr, st
        flat, off = _pack(txs)
        cid = np.frombuffer(_be(chain_id) + b"\0", np.uint8)
        check(_lib.load().gsv_tx_sender_batch(self._h, _ptr(flat), _ptr(off), n, _ptr(cid),
                                              len(_be(chain_id)), int(signer_kind), _ptr(addr),
                                              _ptr(st)))
        return addr, st

    def synth_sign(self, seed: int, n: int, want_pub=True, want_addr=True):
        msg = np.zeros((n, 32), np.uint8)
        sig = np.zeros((n, 65), np.uint8)
        pub = np.zeros((n, 65), np.uint8) if want_pub else None
        addr = np.zeros((n, 20), np.uint8) if want_addr else None
        if n:
            check(_lib.load().gsv_synth_sign(self._h, ctypes.c_uint64(seed), n, _ptr(msg), _ptr(sig),
                                             _ptr(pub), _ptr(addr)))
        return msg, sig, pub, addr

    # -------------------------------------------------------------- device-resident (torch) paths
    def ecrecover_batch_dev(self, msg_t, sig_t, pub_t, addr_t, st_t, stream=None):
        """torch uint8 CUDA tensors already in HBM; enqueues on `stream` (torch stream or None)."""
        n = msg_t.shape[0]
        sp = _sp(stream)
        check(_lib.load().gsv_ecrecover_batch_dev(
            self._h, ctypes.c_void_p(msg_t.data_ptr()), ctypes.c_void_p(sig_t.data_ptr()), n,
            ctypes.c_void_p(pub_t.data_ptr()) if pub_t is not None else None,
            ctypes.c_void_p(addr_t.data_ptr()) if addr_t is not None else None,
            ctypes.c_void_p(st_t.data_ptr()), sp))

    def synth_sign_dev(self, seed, msg_t, sig_t, pub_t=None, addr_t=None, stream=None):
        n = msg_t.shape[0]
        sp = _sp(stream)
        check(_lib.load().gsv_synth_sign_dev(
            self._h, ctypes.c_uint64(seed), n, ctypes.c_void_p(msg_t.data_ptr()),
            ctypes.c_void_p(sig_t.data_ptr()),
            ctypes.c_void_p(pub_t.data_ptr()) if pub_t is not None else None,
            ctypes.c_void_p(addr_t.data_ptr()) if addr_t is not None else None, sp))

    def keccak256_batch_dev(self, data_t, off_t, out_t, stream=None):
        n = out_t.shape[0]
        sp = _sp(stream)
        check(_lib.load().gsv_keccak256_batch_dev(self._h, ctypes.c_void_p(data_t.data_ptr()),
                                                  ctypes.c_void_p(off_t.data_ptr()), n,
                                                  ctypes.c_void_p(out_t.data_ptr()), sp))

    def sha256_batch_dev(self, data_t, off_t, out_t, stream=None):
        """torch CUDA tensors: data_t uint8 messages back to back, off_t (n+1,) int64 offsets into it, out_t
        (n,32) uint8; only enqueues on `stream`."""
        check(_lib.load().gsv_sha256_batch_dev(self._h, ctypes.c_void_p(data_t.data_ptr()),
                                               ctypes.c_void_p(off_t.data_ptr()), out_t.shape[0],
                                               ctypes.c_void_p(out_t.data_ptr()), _sp(stream)))

    def ripemd160_batch_dev(self, data_t, off_t, out_t, stream=None):
        """As sha256_batch_dev; row i of out_t is 12 zero bytes and the 20-byte digest."""
        check(_lib.load().gsv_ripemd160_batch_dev(self._h, ctypes.c_void_p(data_t.data_ptr()),
                                                  ctypes.c_void_p(off_t.data_ptr()), out_t.shape[0],
                                                  ctypes.c_void_p(out_t.data_ptr()), _sp(stream)))


def _be(x: int) -> bytes:
    return x.to_bytes((x.bit_length() + 7) // 8, "big") if x else b""


_default = None
_default_lock = threading.Lock()
_live = weakref.WeakSet()


@atexit.register
def _close_all():
    """Interpreter exit: close every live context (its streams, shapes, communicator) while the HIP
    runtime is intact.  r05 record: a process that left CU-masked streams and the default context to
    static destructors died with SIGSEGV in __cxa_finalize after rocprofv3's finalisation
    (VERDICT r05 weak 1)."""
    global _default
    for c in list(_live):
        try:
            c.close()
        except Exception:
            pass
    _default = None


def default_context() -> Context:
    """Process-wide context on LOCAL_RANK's device (one process per GPU), created on first use,
    like the reference's global secp256k1 context (crypto/secp256k1/secp256.go:45-52)."""
    global _default
    with _default_lock:
        if _default is None:
            dev = int(os.environ.get("LOCAL_RANK", "0"))
            n = device_count()
            if n <= 0:
                raise GsvError("no HIP device visible: libgsv requires an MI355X (gfx950)")
            _default = Context(dev % n)
    return _default


def _chunk_root_batch(self, bodies) -> np.ndarray:
    """DeriveSha(Chunks(body)) for each body (sharding/collation.go:115-119)."""
    n = len(bodies)
    out = np.zeros((n, 32), np.uint8)
    if n == 0:
        return out
    flat, off = _pack(bodies)
    check(_lib.load().gsv_chunk_root_batch(self._h, _ptr(flat), _ptr(off), n, _ptr(out)))
    return out


def _chunk_root_prepare(self, h_off):
    """gsv_chunk_root_prepare: trie plans, device offset table and workspace for these offsets."""
    h_off = np.ascontiguousarray(h_off, np.uint64)
    check(_lib.load().gsv_chunk_root_prepare(self._h, _ptr(h_off), h_off.shape[0] - 1))


def _chunk_root_batch_dev(self, bodies_t, h_off, roots_t, stream=None, prepare=True):
    """bodies_t: torch uint8 CUDA tensor holding all bodies; h_off: numpy uint64 offsets (n+1).
    prepare=False skips the (idempotent, host-side) gsv_chunk_root_prepare: the call then only
    enqueues (graph-capturable) and raises GSV_E_NOT_PREPARED if the offsets were never prepared."""
    h_off = np.ascontiguousarray(h_off, np.uint64)
    n = h_off.shape[0] - 1
    if prepare:
        _chunk_root_prepare(self, h_off)
    sp = _sp(stream)
    check(_lib.load().gsv_chunk_root_batch_dev(self._h, ctypes.c_void_p(bodies_t.data_ptr()), _ptr(h_off), n,
                                               ctypes.c_void_p(roots_t.data_ptr()), sp))


def _pairing_check_batch(self, inputs) -> np.ndarray:
    """bn256Pairing precompile inputs (k x 192 bytes each) -> verdicts GSV_PAIRING_FALSE / TRUE /
    BAD_INPUT (core/vm/contracts.go:333-360, crypto/bn256/cloudflare/bn256.go:313-327)."""
    n = len(inputs)
    out = np.zeros(n, np.uint8)
    if n == 0:
        return out
    flat, off = _pack(inputs)
    check(_lib.load().gsv_bn256_pairing_check_batch(self._h, _ptr(flat), _ptr(off), n, _ptr(out)))
    return out


def _pairing_prepare(self, h_off):
    h_off = np.ascontiguousarray(h_off, np.uint64)
    check(_lib.load().gsv_bn256_pairing_prepare(self._h, _ptr(h_off), h_off.shape[0] - 1))


def _pairing_check_batch_dev(self, in_t, h_off, verdict_t, stream=None, prepare=True):
    """in_t: torch uint8 CUDA tensor with all checks; h_off: numpy uint64 offsets (n+1)."""
    h_off = np.ascontiguousarray(h_off, np.uint64)
    n = h_off.shape[0] - 1
    if prepare:
        _pairing_prepare(self, h_off)
    sp = _sp(stream)
    check(_lib.load().gsv_bn256_pairing_check_batch_dev(self._h, ctypes.c_void_p(in_t.data_ptr()), _ptr(h_off),
                                                        n, ctypes.c_void_p(verdict_t.data_ptr()), sp))


def _bn256_synth_checks_dev(self, seed, out_t, expect_t=None, stream=None):
    """configs[4] synthetic 4-pair checks into out_t (torch uint8 CUDA, nchecks x 768)."""
    n = out_t.shape[0]
    sp = _sp(stream)
    check(_lib.load().gsv_bn256_synth_checks_dev(
        self._h, ctypes.c_uint64(seed), n, ctypes.c_void_p(out_t.data_ptr()),
        ctypes.c_void_p(expect_t.data_ptr()) if expect_t is not None else None, sp))


def _sp(stream):
    """HIP stream handle for a *_dev call: None = the context's own stream.  torch's default (null)
    stream has handle 0, which the C ABI reads as "the context stream" — refused here, because the call
    would then run unordered with the caller's work on that stream."""
    if stream is None:
        return None
    h = int(stream.cuda_stream)
    if h == 0:
        raise ValueError("gsv: pass a non-default torch.cuda.Stream (or None for the context stream); "
                         "the null stream's handle 0 means the context stream in the C ABI")
    return ctypes.c_void_p(h)


def _tptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _notary_validate_shards(self, bodies, chain_id: int = 1, signer_kind: int = _lib.SIGNER_EIP155,
                            max_txs: int = 8192, want_senders=True, want_status=True):
    """Notary validation of collation bodies (gsv.h gsv_notary_validate_shards): returns
    (roots (n,32), ntx (n,), bitmap (n, ceil(max_txs/8)), senders (n,max_txs,20) | None,
    status (n,max_txs) | None)."""
    n = len(bodies)
    bm = (max_txs + 7) // 8
    roots = np.zeros((n, 32), np.uint8)
    ntx = np.zeros(n, np.uint32)
    bitmap = np.zeros((n, bm), np.uint8)
    senders = np.zeros((n, max_txs, 20), np.uint8) if want_senders else None
    status = np.zeros((n, max_txs), np.uint8) if want_status else None
    if n == 0:
        return roots, ntx, bitmap, senders, status
    flat, off = _pack(bodies)
    cid = _be(chain_id)
    cbuf = np.frombuffer(cid + b"\0", np.uint8)
    check(_lib.load().gsv_notary_validate_shards(self._h, _ptr(flat), _ptr(off), n, _ptr(cbuf), len(cid),
                                                 int(signer_kind), int(max_txs), _ptr(roots), _ptr(ntx),
                                                 _ptr(bitmap), _ptr(senders), _ptr(status)))
    return roots, ntx, bitmap, senders, status


def _notary_prepare(self, h_off, chain_id: int = 1, signer_kind: int = _lib.SIGNER_EIP155, max_txs: int = 8192):
    h_off = np.ascontiguousarray(h_off, np.uint64)
    cid = _be(chain_id)
    cbuf = np.frombuffer(cid + b"\0", np.uint8)
    check(_lib.load().gsv_notary_prepare(self._h, _ptr(h_off), h_off.shape[0] - 1, _ptr(cbuf), len(cid),
                                         int(signer_kind), int(max_txs)))


def _notary_validate_shards_dev(self, bodies_t, h_off, roots_t, ntx_t, bitmap_t, senders_t=None, status_t=None,
                                chain_id: int = 1, signer_kind: int = _lib.SIGNER_EIP155, max_txs: int = 8192,
                                stream=None, prepare=True):
    h_off = np.ascontiguousarray(h_off, np.uint64)
    n = h_off.shape[0] - 1
    if prepare:
        _notary_prepare(self, h_off, chain_id, signer_kind, max_txs)
    cid = _be(chain_id)
    cbuf = np.frombuffer(cid + b"\0", np.uint8)
    sp = _sp(stream)
    check(_lib.load().gsv_notary_validate_shards_dev(self._h, _tptr(bodies_t), _ptr(h_off), n, _ptr(cbuf), len(cid),
                                                     int(signer_kind), int(max_txs), _tptr(roots_t), _tptr(ntx_t),
                                                     _tptr(bitmap_t), _tptr(senders_t), _tptr(status_t), sp))


def _notary_synth_dev(self, seed, shard0, n_shards, txs_per_shard, bodies_t, exp_status_t=None, exp_sender_t=None,
                      stream=None):
    sp = _sp(stream)
    check(_lib.load().gsv_notary_synth_dev(self._h, ctypes.c_uint64(seed), int(shard0), int(n_shards),
                                           int(txs_per_shard), _tptr(bodies_t), _tptr(exp_status_t),
                                           _tptr(exp_sender_t), sp))


def comm_unique_id() -> bytes:
    """An RCCL unique id (gsv.h gsv_comm_unique_id): rank 0 creates it and sends it to the others."""
    buf = np.zeros(128, np.uint8)
    check(_lib.load().gsv_comm_unique_id(_ptr(buf)))
    return buf.tobytes()


def shard_range(n_shards: int, nranks: int, rank: int):
    """(first, count) of rank's contiguous shard block (gsv.h gsv_shard_range)."""
    first, count = ctypes.c_size_t(), ctypes.c_size_t()
    check(_lib.load().gsv_shard_range(n_shards, nranks, rank, ctypes.byref(first), ctypes.byref(count)))
    return first.value, count.value


def _comm_init(self, uid: bytes, nranks: int, rank: int):
    buf = np.frombuffer(bytes(uid), np.uint8).copy()
    check(_lib.load().gsv_comm_init(self._h, _ptr(buf), int(nranks), int(rank)))


def _comm_info(self):
    n, r = ctypes.c_int(), ctypes.c_int()
    check(_lib.load().gsv_comm_info(self._h, ctypes.byref(n), ctypes.byref(r)))
    return n.value, r.value


def _notary_validate_partition(self, my_bodies, n_total: int, chain_id: int = 1,
                               signer_kind: int = _lib.SIGNER_EIP155, max_txs: int = 8192,
                               want_senders=False, want_status=False):
    """gsv.h gsv_notary_validate_partition: this rank's block of bodies in, every shard's record out:
    (roots (S,32), ntx (S,), bitmap (S, ceil(max_txs/8)), senders | None, status | None) — the last
    two for this rank's shards only."""
    n = len(my_bodies)
    bm = (max_txs + 7) // 8
    roots = np.zeros((n_total, 32), np.uint8)
    ntx = np.zeros(n_total, np.uint32)
    bitmap = np.zeros((n_total, bm), np.uint8)
    senders = np.zeros((n, max_txs, 20), np.uint8) if want_senders and n else None
    status = np.zeros((n, max_txs), np.uint8) if want_status and n else None
    flat, off = _pack(my_bodies) if n else (np.zeros(1, np.uint8), np.zeros(1, np.uint64))
    cbuf = np.frombuffer(_be(chain_id) + b"\0", np.uint8)
    check(_lib.load().gsv_notary_validate_partition(self._h, _ptr(flat), _ptr(off), n_total, _ptr(cbuf),
                                                    len(_be(chain_id)), int(signer_kind), int(max_txs), _ptr(roots),
                                                    _ptr(ntx), _ptr(bitmap), _ptr(senders), _ptr(status)))
    return roots, ntx, bitmap, senders, status


def partition_block_bytes(n_total: int, nranks: int, max_txs: int = 8192) -> int:
    """Bytes of one rank's record block (gsv.h gsv_partition_block_bytes)."""
    return int(_lib.load().gsv_partition_block_bytes(n_total, nranks, max_txs))


def _notary_partition_prepare(self, h_off, n_total: int, nranks: int, rank: int, chain_id: int = 1,
                              signer_kind: int = _lib.SIGNER_EIP155, max_txs: int = 8192):
    h_off = np.ascontiguousarray(h_off, np.uint64)
    cbuf = np.frombuffer(_be(chain_id) + b"\0", np.uint8)
    check(_lib.load().gsv_notary_partition_prepare(self._h, _ptr(h_off), n_total, int(nranks), int(rank), _ptr(cbuf),
                                                   len(_be(chain_id)), int(signer_kind), int(max_txs)))


def _notary_validate_partition_dev(self, bodies_t, h_off, n_total: int, roots_t, ntx_t, bitmap_t, senders_t=None,
                                   status_t=None, rank_status_t=None, chain_id: int = 1,
                                   signer_kind: int = _lib.SIGNER_EIP155, max_txs: int = 8192, stream=None,
                                   prepare=True):
    """gsv.h gsv_notary_validate_partition_dev: this rank's block (HBM, host offsets h_off) in; every
    shard's record out in HBM (validation + pack + one ncclAllGather + unpack on `stream`)."""
    h_off = np.ascontiguousarray(h_off, np.uint64)
    if prepare:
        n, r = self.comm_info()
        _notary_partition_prepare(self, h_off, n_total, n, r, chain_id, signer_kind, max_txs)
    cbuf = np.frombuffer(_be(chain_id) + b"\0", np.uint8)
    sp = _sp(stream)
    check(_lib.load().gsv_notary_validate_partition_dev(
        self._h, _tptr(bodies_t), _ptr(h_off), n_total, _ptr(cbuf), len(_be(chain_id)), int(signer_kind),
        int(max_txs), _tptr(roots_t), _tptr(ntx_t), _tptr(bitmap_t), _tptr(senders_t), _tptr(status_t),
        _tptr(rank_status_t), sp))


def _notary_partition_pack_dev(self, bodies_t, h_off, n_total: int, nranks: int, rank: int, block_t,
                               senders_t=None, status_t=None, chain_id: int = 1,
                               signer_kind: int = _lib.SIGNER_EIP155, max_txs: int = 8192, stream=None, prepare=True):
    """gsv.h gsv_notary_partition_pack_dev: validate rank `rank`'s block and write its record block."""
    h_off = np.ascontiguousarray(h_off, np.uint64)
    if prepare:
        _notary_partition_prepare(self, h_off, n_total, nranks, rank, chain_id, signer_kind, max_txs)
    cbuf = np.frombuffer(_be(chain_id) + b"\0", np.uint8)
    sp = _sp(stream)
    check(_lib.load().gsv_notary_partition_pack_dev(
        self._h, _tptr(bodies_t), _ptr(h_off), n_total, int(nranks), int(rank), _ptr(cbuf), len(_be(chain_id)),
        int(signer_kind), int(max_txs), _tptr(block_t), _tptr(senders_t), _tptr(status_t), sp))


def _notary_partition_unpack_dev(self, blocks_t, n_total: int, nranks: int, roots_t, ntx_t, bitmap_t,
                                 rank_status_t=None, max_txs: int = 8192, stream=None):
    """gsv.h gsv_notary_partition_unpack_dev: nranks gathered blocks (rank order) -> shard-order records."""
    sp = _sp(stream)
    check(_lib.load().gsv_notary_partition_unpack_dev(self._h, _tptr(blocks_t), n_total, int(nranks), int(max_txs),
                                                      _tptr(roots_t), _tptr(ntx_t), _tptr(bitmap_t),
                                                      _tptr(rank_status_t), sp))


Context.notary_partition_prepare = _notary_partition_prepare
Context.notary_validate_partition_dev = _notary_validate_partition_dev
Context.notary_partition_pack_dev = _notary_partition_pack_dev
Context.notary_partition_unpack_dev = _notary_partition_unpack_dev
Context.comm_init = _comm_init
Context.comm_info = _comm_info
Context.notary_validate_partition = _notary_validate_partition
Context.notary_prepare = _notary_prepare
Context.chunk_root_prepare = _chunk_root_prepare
Context.pairing_prepare = _pairing_prepare
Context.notary_validate_shards = _notary_validate_shards
Context.notary_validate_shards_dev = _notary_validate_shards_dev
Context.notary_synth_dev = _notary_synth_dev
Context.bn256_synth_checks_dev = _bn256_synth_checks_dev
Context.pairing_check_batch = _pairing_check_batch
Context.pairing_check_batch_dev = _pairing_check_batch_dev
Context.chunk_root_batch = _chunk_root_batch
Context.chunk_root_batch_dev = _chunk_root_batch_dev


def _derive_sha_batch(self, lists) -> np.ndarray:
    """types.DeriveSha for each list of item RLPs (core/types/derive_sha.go:32-41): list i is a
    sequence of byte strings, item j being list.GetRlp(j) (rlp(tx) for a block's transactions)."""
    n = len(lists)
    out = np.zeros((n, 32), np.uint8)
    if n == 0:
        return out
    items = [bytes(x) for lst in lists for x in lst]
    flat, voff = _pack(items)
    list_off = np.zeros(n + 1, np.uint64)
    list_off[1:] = np.cumsum([len(lst) for lst in lists])
    check(_lib.load().gsv_derive_sha_batch(self._h, _ptr(flat), _ptr(voff), _ptr(list_off), n, _ptr(out)))
    return out


def _derive_sha_prepare(self, voff, list_off):
    voff = np.ascontiguousarray(voff, np.uint64)
    list_off = np.ascontiguousarray(list_off, np.uint64)
    check(_lib.load().gsv_derive_sha_prepare(self._h, _ptr(voff), _ptr(list_off), list_off.shape[0] - 1))


def _derive_sha_batch_dev(self, vals_t, voff, list_off, roots_t, stream=None, prepare=True):
    """vals_t: torch uint8 CUDA tensor of all item bytes; voff (items+1) / list_off (lists+1): numpy uint64."""
    voff = np.ascontiguousarray(voff, np.uint64)
    list_off = np.ascontiguousarray(list_off, np.uint64)
    n = list_off.shape[0] - 1
    if prepare:
        _derive_sha_prepare(self, voff, list_off)
    sp = _sp(stream)
    check(_lib.load().gsv_derive_sha_batch_dev(self._h, _tptr(vals_t), _ptr(voff), _ptr(list_off), n,
                                               _tptr(roots_t), sp))


def _collation_poc_batch(self, bodies, salt: bytes) -> np.ndarray:
    """Collation.CalculatePOC(salt) for each body (sharding/collation.go:124-136)."""
    n = len(bodies)
    out = np.zeros((n, 32), np.uint8)
    if n == 0:
        return out
    flat, off = _pack(bodies)
    sb = np.frombuffer(bytes(salt) + b"\0", np.uint8)
    check(_lib.load().gsv_collation_poc_batch(self._h, _ptr(flat), _ptr(off), n, _ptr(sb), len(salt), _ptr(out)))
    return out


def _collation_poc_prepare(self, h_off, salt: bytes):
    h_off = np.ascontiguousarray(h_off, np.uint64)
    sb = np.frombuffer(bytes(salt) + b"\0", np.uint8)
    check(_lib.load().gsv_collation_poc_prepare(self._h, _ptr(h_off), h_off.shape[0] - 1, _ptr(sb), len(salt)))


def _collation_poc_batch_dev(self, bodies_t, h_off, salt: bytes, out_t, stream=None, prepare=True):
    h_off = np.ascontiguousarray(h_off, np.uint64)
    n = h_off.shape[0] - 1
    if prepare:
        _collation_poc_prepare(self, h_off, salt)
    sb = np.frombuffer(bytes(salt) + b"\0", np.uint8)
    sp = _sp(stream)
    check(_lib.load().gsv_collation_poc_batch_dev(self._h, _tptr(bodies_t), _ptr(h_off), n, _ptr(sb), len(salt),
                                                  _tptr(out_t), sp))


def _collation_header_verify_batch(self, shard_id32, chunk_root32, period32, proposer20, sig65, nil_flags=None):
    """Collation header hashes + proposer-signature check (gsv.h gsv_collation_header_verify_batch):
    returns (hash32 (n,32), signer20 (n,20), status (n,))."""
    sid = _np_u8(shard_id32).reshape(-1, 32)
    n = sid.shape[0]
    root = _np_u8(chunk_root32).reshape(n, 32)
    per = _np_u8(period32).reshape(n, 32)
    prop = _np_u8(proposer20).reshape(n, 20)
    sig = _np_u8(sig65).reshape(n, 65)
    nf = None if nil_flags is None else _np_u8(nil_flags).reshape(n)
    h = np.zeros((n, 32), np.uint8)
    signer = np.zeros((n, 20), np.uint8)
    st = np.zeros(n, np.uint8)
    if n == 0:
        return h, signer, st
    check(_lib.load().gsv_collation_header_verify_batch(self._h, _ptr(sid), _ptr(root), _ptr(per), _ptr(prop),
                                                        _ptr(sig), _ptr(nf) if nf is not None else None, n,
                                                        _ptr(h), _ptr(signer), _ptr(st)))
    return h, signer, st


def _collation_header_verify_batch_dev(self, sid_t, root_t, per_t, prop_t, sig_t, st_t, nil_t=None, hash_t=None,
                                       signer_t=None, stream=None, prepare=True):
    n = sid_t.shape[0]
    if prepare:
        check(_lib.load().gsv_collation_header_prepare(self._h, n))
    sp = _sp(stream)
    check(_lib.load().gsv_collation_header_verify_batch_dev(self._h, _tptr(sid_t), _tptr(root_t), _tptr(per_t),
                                                            _tptr(prop_t), _tptr(sig_t), _tptr(nil_t), n,
                                                            _tptr(hash_t), _tptr(signer_t), _tptr(st_t), sp))


Context.collation_header_verify_batch_dev = _collation_header_verify_batch_dev
Context.derive_sha_batch = _derive_sha_batch
Context.derive_sha_batch_dev = _derive_sha_batch_dev
Context.collation_poc_batch = _collation_poc_batch
Context.collation_poc_batch_dev = _collation_poc_batch_dev
Context.collation_header_verify_batch = _collation_header_verify_batch
Context.derive_sha_prepare = _derive_sha_prepare
Context.collation_poc_prepare = _collation_poc_prepare


def _ecrecover_precompile_batch(self, inputs):
    """The ecrecover precompile's Run over many inputs (core/vm/contracts.go:78-101): returns
    (out32 (n,32), ok (n,)); ok[i] == 0 where the reference returns (nil, nil)."""
    n = len(inputs)
    out = np.zeros((n, 32), np.uint8)
    ok = np.zeros(n, np.uint8)
    if n == 0:
        return out, ok
    flat, off = _pack(inputs)
    check(_lib.load().gsv_ecrecover_precompile_batch(self._h, _ptr(flat), _ptr(off), n, _ptr(out), _ptr(ok)))
    return out, ok


def _ecrecover_precompile_batch_dev(self, in_t, out_t, ok_t, stream=None):
    """in_t: torch uint8 CUDA tensor (n, 128) of right-padded precompile inputs."""
    n = in_t.shape[0]
    sp = _sp(stream)
    check(_lib.load().gsv_ecrecover_precompile_batch_dev(self._h, _tptr(in_t), n, _tptr(out_t), _tptr(ok_t), sp))


def _bn256_g1_batch(self, fn, inputs):
    n = len(inputs)
    out = np.zeros((n, 64), np.uint8)
    st = np.zeros(n, np.uint8)
    if n == 0:
        return out, st
    flat, off = _pack(inputs)
    check(fn(self._h, _ptr(flat), _ptr(off), n, _ptr(out), _ptr(st)))
    return out, st


def _bn256_add_batch(self, inputs):
    """The bn256Add precompile's Run over many inputs (core/vm/contracts.go:274-289): returns
    (out64 (n,64), status (n,)); status[i] == ST_BN_BAD_INPUT (and a zero row) where the reference
    returns the unmarshal error."""
    return _bn256_g1_batch(self, _lib.load().gsv_bn256_add_batch, inputs)


def _bn256_scalar_mul_batch(self, inputs):
    """The bn256ScalarMul precompile's Run over many inputs (core/vm/contracts.go:297-312): returns
    (out64 (n,64), status (n,)) as bn256_add_batch does."""
    return _bn256_g1_batch(self, _lib.load().gsv_bn256_scalar_mul_batch, inputs)


def _bn256_add_batch_dev(self, in_t, out_t, st_t, stream=None):
    """in_t: torch uint8 CUDA tensor (n, 128) of right-padded records; out_t (n, 64), st_t (n,)."""
    n = in_t.shape[0]
    sp = _sp(stream)
    check(_lib.load().gsv_bn256_add_batch_dev(self._h, _tptr(in_t), n, _tptr(out_t), _tptr(st_t), sp))


def _bn256_scalar_mul_batch_dev(self, in_t, out_t, st_t, stream=None):
    """in_t: torch uint8 CUDA tensor (n, 96) of right-padded records; out_t (n, 64), st_t (n,)."""
    n = in_t.shape[0]
    sp = _sp(stream)
    check(_lib.load().gsv_bn256_scalar_mul_batch_dev(self._h, _tptr(in_t), n, _tptr(out_t), _tptr(st_t), sp))


def _ecdsa_verify_batch(self, msgs, sigs, pubkeys):
    """ECDSA verification with known keys (gsv.h gsv_ecdsa_verify_batch, the reference's
    secp256k1.VerifySignature): msgs (n,32) uint8, sigs (n,64) uint8 [R || S], pubkeys a list of n byte
    strings of any length (33-byte compressed and 65-byte uncompressed or hybrid keys parse).  Returns
    ok (n,) uint8: 1 where the signature is valid, in lower-s form, and made by that key."""
    msgs = np.ascontiguousarray(msgs, np.uint8).reshape(-1, 32)
    sigs = np.ascontiguousarray(sigs, np.uint8).reshape(-1, 64)
    n = msgs.shape[0]
    if sigs.shape[0] != n or len(pubkeys) != n:
        raise ValueError("msgs, sigs and pubkeys batch sizes differ")
    ok = np.zeros(n, np.uint8)
    if n:
        flat, off = _pack(pubkeys)
        check(_lib.load().gsv_ecdsa_verify_batch(self._h, _ptr(msgs), _ptr(sigs), _ptr(flat), _ptr(off), n, _ptr(ok)))
    return ok


def _pubkey_parse_batch(self, pubkeys):
    """Parses and re-encodes public keys (gsv.h gsv_pubkey_parse_batch): returns (pub65 (n,65), ok (n,));
    pub65[i] = 04 || X || Y where key i parses, a zero row and ok[i] == 0 where it does not."""
    n = len(pubkeys)
    out = np.zeros((n, 65), np.uint8)
    ok = np.zeros(n, np.uint8)
    if n:
        flat, off = _pack(pubkeys)
        check(_lib.load().gsv_pubkey_parse_batch(self._h, _ptr(flat), _ptr(off), n, _ptr(out), _ptr(ok)))
    return out, ok


def _ecdsa_verify_batch_dev(self, msg_t, sig_t, pub_t, len_t, ok_t, stream=None):
    """torch uint8 CUDA tensors: msg_t (n,32), sig_t (n,64), pub_t (n,65) key rows, len_t (n,) key lengths
    (33 or 65), ok_t (n,); only enqueues on `stream`."""
    n = msg_t.shape[0]
    sp = _sp(stream)
    check(_lib.load().gsv_ecdsa_verify_batch_dev(self._h, _tptr(msg_t), _tptr(sig_t), _tptr(pub_t), _tptr(len_t), n,
                                                 _tptr(ok_t), sp))


def _pubkey_parse_batch_dev(self, pub_t, len_t, out_t, ok_t, stream=None):
    """torch uint8 CUDA tensors: pub_t (n,65) key rows, len_t (n,), out_t (n,65), ok_t (n,)."""
    n = pub_t.shape[0]
    sp = _sp(stream)
    check(_lib.load().gsv_pubkey_parse_batch_dev(self._h, _tptr(pub_t), _tptr(len_t), n, _tptr(out_t), _tptr(ok_t),
                                                 sp))


def _seckey_rows(keys):
    keys = np.ascontiguousarray(keys, np.uint8)
    if keys.size % 32:
        raise ValueError("secret keys are 32 bytes each")
    return keys.reshape(-1, 32)


def _ecdsa_sign_batch(self, msgs, keys):
    """crypto.Sign over a batch (gsv.h gsv_ecdsa_sign_batch): msgs (n,32) uint8 hashes, keys (n,32) uint8
    big-endian secret keys.  Returns (sig65 (n,65) [R || S || recid], status (n,)); status[i] ==
    ST_INVALID_KEY and a zero row for a key of 0 or >= n.  The keys' device copy is overwritten before the
    call returns; the arrays passed in stay the caller's to wipe."""
    msgs = np.ascontiguousarray(msgs, np.uint8).reshape(-1, 32)
    keys = _seckey_rows(keys)
    n = msgs.shape[0]
    if keys.shape[0] != n:
        raise ValueError("msgs and keys batch sizes differ")
    sig = np.zeros((n, 65), np.uint8)
    st = np.zeros(n, np.uint8)
    if n:
        check(_lib.load().gsv_ecdsa_sign_batch(self._h, _ptr(msgs), _ptr(keys), n, _ptr(sig), _ptr(st)))
    return sig, st


def _pubkey_create_batch(self, keys, want_addr=False):
    """Public keys of secret keys (gsv.h gsv_pubkey_create_batch): returns (pub65 (n,65), addr20 (n,20) or
    None, status (n,)); a zero row and ST_INVALID_KEY for a key of 0 or >= n."""
    keys = _seckey_rows(keys)
    n = keys.shape[0]
    pub = np.zeros((n, 65), np.uint8)
    addr = np.zeros((n, 20), np.uint8) if want_addr else None
    st = np.zeros(n, np.uint8)
    if n:
        check(_lib.load().gsv_pubkey_create_batch(self._h, _ptr(keys), n, _ptr(pub),
                                                  _ptr(addr) if want_addr else None, _ptr(st)))
    return pub, addr, st


def _ecdsa_sign_batch_dev(self, msg_t, key_t, sig_t, st_t, stream=None):
    """torch uint8 CUDA tensors: msg_t (n,32), key_t (n,32) secret keys, sig_t (n,65), st_t (n,); only
    enqueues on `stream`.  key_t is the caller's to wipe."""
    n = msg_t.shape[0]
    sp = _sp(stream)
    check(_lib.load().gsv_ecdsa_sign_batch_dev(self._h, _tptr(msg_t), _tptr(key_t), n, _tptr(sig_t), _tptr(st_t), sp))


def _pubkey_create_batch_dev(self, key_t, pub_t, addr_t, st_t, stream=None):
    """torch uint8 CUDA tensors: key_t (n,32), pub_t (n,65), addr_t (n,20) or None, st_t (n,)."""
    n = key_t.shape[0]
    sp = _sp(stream)
    check(_lib.load().gsv_pubkey_create_batch_dev(self._h, _tptr(key_t), n, _tptr(pub_t),
                                                  _tptr(addr_t) if addr_t is not None else None, _tptr(st_t), sp))


def _check_signer(chain_id: int, signer_kind: int) -> bytes:
    if signer_kind not in (_lib.SIGNER_EIP155, _lib.SIGNER_HOMESTEAD, _lib.SIGNER_FRONTIER):
        raise ValueError("signer_kind is one of SIGNER_EIP155, SIGNER_HOMESTEAD, SIGNER_FRONTIER")
    cid = _be(int(chain_id))
    if chain_id < 0 or len(cid) > 64:
        raise ValueError("the chain id is a non-negative integer of at most 64 bytes")
    return cid


def _tx_sign_batch(self, txs, keys, chain_id: int, signer_kind: int, want_hash=True):
    """types.SignTx over a batch (gsv.h gsv_tx_sign_batch): txs = RLP-encoded transactions, signed or not,
    keys (n,32) uint8 big-endian secret keys.  Returns (signed: list of bytes, the RLP of each signed
    transaction, b"" for a failed item; hashes (n,32) uint8 tx.Hash() or None; status (n,)): ST_BAD_RLP for
    what does not decode, ST_INVALID_KEY for a key of 0 or >= n, ST_BODY_TOO_LARGE past 2^20 bytes.  The
    keys' device copy is overwritten before the call returns."""
    cid = _check_signer(chain_id, signer_kind)
    keys = _seckey_rows(keys)
    n = len(txs)
    if keys.shape[0] != n:
        raise ValueError("txs and keys batch sizes differ")
    st = np.zeros(n, np.uint8)
    hashes = np.zeros((n, 32), np.uint8) if want_hash else None
    if n == 0:
        return [], hashes, st
    flat, off = _pack(txs)
    G = _lib.tx_sign_growth(len(cid))
    out = np.zeros(int(off[n]) + n * G, np.uint8)
    olen = np.zeros(n, np.uint32)
    cidb = np.frombuffer(cid + b"\0", np.uint8)
    check(_lib.load().gsv_tx_sign_batch(self._h, _ptr(flat), _ptr(off), n, _ptr(keys), _ptr(cidb), len(cid),
                                        int(signer_kind), _ptr(out), _ptr(olen), _ptr(hashes) if want_hash else None,
                                        _ptr(st)))
    signed = [out[int(off[i]) + i * G:int(off[i]) + i * G + int(olen[i])].tobytes() for i in range(n)]
    return signed, hashes, st


def tx_sign_work_bytes(n: int) -> int:
    """bytes of the work area tx_sign_batch_dev needs (gsv.h gsv_tx_sign_work_bytes)"""
    return int(_lib.load().gsv_tx_sign_work_bytes(n))


def _tx_sign_batch_dev(self, rlp_t, off_t, key_t, chain_id: int, signer_kind: int, out_t, olen_t, hash_t, st_t, work_t,
                       stream=None):
    """torch CUDA tensors: rlp_t uint8 transactions back to back, off_t (n+1,) int64 offsets into it, key_t (n,32)
    secret keys, out_t uint8 of off[n] + n * tx_sign_growth(chain id bytes) bytes (item i at off[i] + i * growth),
    olen_t (n,) int32, hash_t (n,32) uint8 or None, st_t (n,) uint8, work_t uint8 of tx_sign_work_bytes(n) bytes.
    Only enqueues on `stream`: three launches, no allocation.  key_t is the caller's to wipe."""
    cid = _check_signer(chain_id, signer_kind)
    n = key_t.shape[0]
    if off_t.numel() != n + 1 or work_t.numel() < tx_sign_work_bytes(n):
        raise ValueError("off_t holds n + 1 offsets; work_t holds tx_sign_work_bytes(n) bytes")
    cidb = np.frombuffer(cid + b"\0", np.uint8)
    sp = _sp(stream)
    check(_lib.load().gsv_tx_sign_batch_dev(self._h, _tptr(rlp_t), _tptr(off_t), n, _tptr(key_t), _ptr(cidb), len(cid),
                                            int(signer_kind), _tptr(out_t), _tptr(olen_t), _tptr(hash_t), _tptr(st_t),
                                            _tptr(work_t), sp))


def _point_rows(points):
    points = np.ascontiguousarray(points, np.uint8)
    if points.size % 64:
        raise ValueError("points are 64 bytes each (X || Y)")
    return points.reshape(-1, 64)


def _secp256k1_scalar_mul_batch(self, points, scalars):
    """BitCurve.ScalarMult over a batch (gsv.h gsv_secp256k1_scalar_mul_batch): points (n,64) uint8 X || Y,
    scalars (n,32) uint8 big-endian.  Returns (out (n,64) X || Y of k P, status (n,)): ST_INVALID_KEY for a
    scalar of 0 or >= n, ST_INVALID_CURVE for a point off the curve, a zero row for both.  The device copies
    of the scalars and the products are overwritten before the call returns."""
    points = _point_rows(points)
    scalars = _seckey_rows(scalars)
    n = points.shape[0]
    if scalars.shape[0] != n:
        raise ValueError("points and scalars batch sizes differ")
    out = np.zeros((n, 64), np.uint8)
    st = np.zeros(n, np.uint8)
    if n:
        check(_lib.load().gsv_secp256k1_scalar_mul_batch(self._h, _ptr(points), _ptr(scalars), n, _ptr(out), _ptr(st)))
    return out, st


def _ecdh_batch(self, pubs, keys, want_shared=True, want_keys=False):
    """ECDH over a batch (gsv.h gsv_ecdh_batch): pubs (n,64) uint8 public points X || Y, keys (n,32) uint8
    big-endian secret keys.  Returns (shared (n,32) or None, keys48 (n,48) Ke || Km or None, status (n,));
    the statuses and the zero rows are scalar_mul_batch's."""
    if not (want_shared or want_keys):
        raise ValueError("ask for the shared secrets, the derived keys or both")
    pubs = _point_rows(pubs)
    keys = _seckey_rows(keys)
    n = pubs.shape[0]
    if keys.shape[0] != n:
        raise ValueError("pubs and keys batch sizes differ")
    shared = np.zeros((n, 32), np.uint8) if want_shared else None
    k48 = np.zeros((n, 48), np.uint8) if want_keys else None
    st = np.zeros(n, np.uint8)
    if n:
        check(_lib.load().gsv_ecdh_batch(self._h, _ptr(pubs), _ptr(keys), n, _ptr(shared) if want_shared else None,
                                         _ptr(k48) if want_keys else None, _ptr(st)))
    return shared, k48, st


def _secp256k1_scalar_mul_batch_dev(self, pt_t, k_t, out_t, st_t, stream=None):
    """torch uint8 CUDA tensors: pt_t (n,64), k_t (n,32) scalars, out_t (n,64), st_t (n,); only enqueues on
    `stream`.  k_t and out_t are the caller's to wipe."""
    n = pt_t.shape[0]
    sp = _sp(stream)
    check(_lib.load().gsv_secp256k1_scalar_mul_batch_dev(self._h, _tptr(pt_t), _tptr(k_t), n, _tptr(out_t),
                                                         _tptr(st_t), sp))


def _ecdh_batch_dev(self, pub_t, key_t, shared_t, keys_t, st_t, stream=None):
    """torch uint8 CUDA tensors: pub_t (n,64), key_t (n,32) secret keys, shared_t (n,32) or None, keys_t
    (n,48) or None (not both None), st_t (n,); only enqueues on `stream`."""
    n = pub_t.shape[0]
    sp = _sp(stream)
    check(_lib.load().gsv_ecdh_batch_dev(self._h, _tptr(pub_t), _tptr(key_t), n, _tptr(shared_t), _tptr(keys_t),
                                         _tptr(st_t), sp))


def _s2_tables(s2s, n):
    """per-item s2 byte strings (or None: every s2 empty) -> (flat, off) or (None, None)"""
    if s2s is None:
        return None, None
    if len(s2s) != n:
        raise ValueError("one s2 per item (or None)")
    return _pack([b"" if s is None else s for s in s2s])


def _ecies_decrypt_batch(self, cts, keys, s2s=None):
    """ecies.PrivateKey.Decrypt over a batch (gsv.h gsv_ecies_decrypt_batch): cts a list of ciphertexts, keys
    (n,32) uint8 big-endian secret keys, s2s a list of byte strings or None.  Returns (msgs, status (n,)):
    msgs[i] is the message (b"" where the status is not ST_OK).  The device copies of the keys, the derived
    keys and the plaintext are overwritten before the call returns."""
    keys = _seckey_rows(keys)
    n = len(cts)
    if keys.shape[0] != n:
        raise ValueError("cts and keys batch sizes differ")
    flat, off = _pack(cts)
    s2, s2off = _s2_tables(s2s, n)
    out = np.zeros(int(off[-1]) + 1, np.uint8)
    mlen = np.zeros(n, np.uint32)
    st = np.zeros(n, np.uint8)
    if n:
        check(_lib.load().gsv_ecies_decrypt_batch(self._h, _ptr(flat), _ptr(off), _ptr(keys), _ptr(s2), _ptr(s2off), n,
                                                  _ptr(out), _ptr(mlen), _ptr(st)))
    return [out[int(off[i]):int(off[i]) + int(mlen[i])].tobytes() for i in range(n)], st


def _ecies_encrypt_batch(self, msgs, pubs, ephs, ivs, s2s=None):
    """ecies.Encrypt over a batch (gsv.h gsv_ecies_encrypt_batch): msgs a list of messages, pubs (n,64) uint8
    recipient points X || Y, ephs (n,32) ephemeral secret keys, ivs (n,16).  Returns (cts, status (n,)): cts[i]
    is 04 || R || iv || ciphertext || tag (113 + len(m) zero bytes where the status is not ST_OK)."""
    pubs = _point_rows(pubs)
    ephs = _seckey_rows(ephs)
    ivs = np.ascontiguousarray(ivs, np.uint8).reshape(-1, 16)
    n = len(msgs)
    if not (pubs.shape[0] == ephs.shape[0] == ivs.shape[0] == n):
        raise ValueError("msgs, pubs, ephs and ivs batch sizes differ")
    flat, off = _pack(msgs)
    s2, s2off = _s2_tables(s2s, n)
    out = np.zeros(int(off[-1]) + _lib.ECIES_OVERHEAD * n, np.uint8)
    st = np.zeros(n, np.uint8)
    if n:
        check(_lib.load().gsv_ecies_encrypt_batch(self._h, _ptr(flat), _ptr(off), _ptr(pubs), _ptr(ephs), _ptr(ivs),
                                                  _ptr(s2), _ptr(s2off), n, _ptr(out), _ptr(st)))
    pos = [int(off[i]) + _lib.ECIES_OVERHEAD * i for i in range(n + 1)]
    return [out[pos[i]:pos[i + 1]].tobytes() for i in range(n)], st


def ecies_work_bytes(n: int, encrypt: bool) -> int:
    """bytes of the work area the ecies *_dev forms need (gsv.h gsv_ecies_work_bytes)"""
    return int(_lib.load().gsv_ecies_work_bytes(n, 1 if encrypt else 0))


def _ecies_decrypt_batch_dev(self, ct_t, ct_off_t, key_t, s2_t, s2_off_t, msg_t, mlen_t, st_t, work_t, stream=None):
    """torch CUDA tensors: ct_t uint8 ciphertexts back to back, ct_off_t (n+1,) int64 offsets into it, key_t (n,32),
    s2_t / s2_off_t likewise or both None, msg_t uint8 (the slots: as long as ct_t), mlen_t (n,) int32, st_t (n,)
    uint8, work_t uint8 of ecies_work_bytes(n, False) bytes (left all zero).  Only enqueues on `stream`."""
    n = key_t.shape[0]
    if ct_off_t.numel() != n + 1 or work_t.numel() < ecies_work_bytes(n, False):
        raise ValueError("ct_off_t holds n + 1 offsets; work_t holds ecies_work_bytes(n, False) bytes")
    sp = _sp(stream)
    check(_lib.load().gsv_ecies_decrypt_batch_dev(self._h, _tptr(ct_t), _tptr(ct_off_t), _tptr(key_t), _tptr(s2_t),
                                                  _tptr(s2_off_t), n, _tptr(msg_t), _tptr(mlen_t), _tptr(st_t),
                                                  _tptr(work_t), sp))


def _ecies_encrypt_batch_dev(self, msg_t, msg_off_t, pub_t, eph_t, iv_t, s2_t, s2_off_t, ct_t, st_t, work_t, stream=None):
    """torch CUDA tensors: msg_t uint8 messages back to back, msg_off_t (n+1,) int64, pub_t (n,64), eph_t (n,32),
    iv_t (n,16), s2_t / s2_off_t or both None, ct_t uint8 (item i at msg_off[i] + 113 i), st_t (n,), work_t uint8
    of ecies_work_bytes(n, True) bytes (left all zero).  Only enqueues on `stream`."""
    n = pub_t.shape[0]
    if msg_off_t.numel() != n + 1 or work_t.numel() < ecies_work_bytes(n, True):
        raise ValueError("msg_off_t holds n + 1 offsets; work_t holds ecies_work_bytes(n, True) bytes")
    sp = _sp(stream)
    check(_lib.load().gsv_ecies_encrypt_batch_dev(self._h, _tptr(msg_t), _tptr(msg_off_t), _tptr(pub_t), _tptr(eph_t),
                                                  _tptr(iv_t), _tptr(s2_t), _tptr(s2_off_t), n, _tptr(ct_t), _tptr(st_t),
                                                  _tptr(work_t), sp))


def modexp_output_layout(inputs):
    """(out_off uint64[n+1], status uint8[n]) of a batch of modexp precompile inputs (gsv.h
    gsv_modexp_output_layout; host only): item i's output is out_off[i+1] - out_off[i] = modLen_i bytes, 0
    with ST_MODEXP_TOO_LONG when one of its lengths is above MODEXP_MAX_LEN."""
    n = len(inputs)
    flat, off = _pack(inputs)
    out_off = np.zeros(n + 1, np.uint64)
    st = np.zeros(n, np.uint8)
    check(_lib.load().gsv_modexp_output_layout(_ptr(flat), _ptr(off), n, _ptr(out_off), _ptr(st)))
    return out_off, st


def _modexp_batch(self, inputs):
    """The bigModExp precompile (0x05) over a batch (gsv.h gsv_modexp_batch): inputs as the precompile
    receives them.  Returns (outputs: list of bytes, modLen_i bytes each; status (n,) uint8: ST_OK, or
    ST_MODEXP_TOO_LONG with an empty output for an item with a length above MODEXP_MAX_LEN)."""
    inputs = [bytes(x) for x in inputs]
    n = len(inputs)
    if n == 0:
        return [], np.zeros(0, np.uint8)
    flat, off = _pack(inputs)
    out_off = np.zeros(n + 1, np.uint64)
    st = np.zeros(n, np.uint8)
    L = _lib.load()
    check(L.gsv_modexp_output_layout(_ptr(flat), _ptr(off), n, _ptr(out_off), _ptr(st)))
    out = np.zeros(int(out_off[n]) + 8, np.uint8)
    check(L.gsv_modexp_batch(self._h, _ptr(flat), _ptr(off), n, _ptr(out), _ptr(out_off), _ptr(st)))
    return [out[int(out_off[i]):int(out_off[i + 1])].tobytes() for i in range(n)], st


def modexp_work_bytes(n: int, base_len: int, exp_len: int, mod_len: int) -> int:
    """bytes of the work buffer modexp_batch_dev needs for this shape (gsv.h gsv_modexp_work_bytes)"""
    return int(_lib.load().gsv_modexp_work_bytes(int(n), int(base_len), int(exp_len), int(mod_len)))


def _modexp_batch_dev(self, in_t, base_len: int, exp_len: int, mod_len: int, out_t, work_t=None, stream=None):
    """torch CUDA uint8 tensors: in_t (n, base_len + exp_len + mod_len) rows of base || exp || mod (any byte
    alignment), out_t (n, mod_len), work_t of modexp_work_bytes(...) bytes, 4-byte aligned (None where that is
    0).  Only enqueues on `stream`: one launch, no allocation."""
    for v in (base_len, exp_len, mod_len):
        if not 0 <= int(v) <= _lib.MODEXP_MAX_LEN:
            raise ValueError("modexp: each length is at most MODEXP_MAX_LEN bytes")
    row = int(base_len) + int(exp_len) + int(mod_len)
    n = int(in_t.shape[0])
    if not in_t.is_contiguous() or not out_t.is_contiguous() or in_t.numel() != n * row or \
            out_t.numel() != n * int(mod_len):
        raise ValueError("in_t is n contiguous rows of base_len + exp_len + mod_len bytes, out_t n rows of mod_len")
    need = modexp_work_bytes(n, base_len, exp_len, mod_len)
    if need and (work_t is None or work_t.numel() * work_t.element_size() < need):
        raise ValueError("work_t holds modexp_work_bytes(n, base_len, exp_len, mod_len) bytes")
    sp = _sp(stream)
    check(_lib.load().gsv_modexp_batch_dev(self._h, _tptr(in_t), n, int(base_len), int(exp_len), int(mod_len),
                                           _tptr(out_t), _tptr(work_t), sp))


def _rows32(a) -> np.ndarray:
    """(n, 32) uint8 from an array, one bytes object, or a sequence of 32-byte strings"""
    if isinstance(a, (list, tuple)) and (not a or isinstance(a[0], (bytes, bytearray, memoryview))):
        a = b"".join(bytes(x) for x in a)
    a = np.ascontiguousarray(_np_u8(a)).reshape(-1, 32)
    return a if a.flags.writeable else a.copy()  # torch.from_numpy wants a writable array


def _ethash_rows(hashes, nonces):
    h = _rows32(hashes)
    nn = np.ascontiguousarray(nonces, np.uint64).reshape(-1)
    if h.shape[0] != nn.shape[0]:
        raise ValueError("ethash: one 32-byte hash and one nonce per item")
    return h, nn


def _ethash_light_batch(self, numbers, hashes, nonces, test_mode=False):
    """hashimotoLight per (block number, hash without nonce, nonce) (gsv.h gsv_ethash_light_batch): items are
    grouped by epoch, the epoch caches are made on the host and kept on the device.  Returns (mix digests
    (n, 32), results (n, 32)) in input order."""
    h, nn = _ethash_rows(hashes, nonces)
    num = np.ascontiguousarray(numbers, np.uint64).reshape(-1)
    n = h.shape[0]
    if num.shape[0] != n:
        raise ValueError("ethash: one block number per item")
    mix = np.zeros((n, 32), np.uint8)
    res = np.zeros((n, 32), np.uint8)
    check(_lib.load().gsv_ethash_light_batch(self._h, _ptr(num), int(bool(test_mode)), _ptr(h), _ptr(nn), n, _ptr(mix),
                                             _ptr(res)))
    return mix, res


def _ethash_verify_seal_batch(self, numbers, hashes, nonces, mixes, difficulties, test_mode=False):
    """VerifySeal's checks per item (gsv.h gsv_ethash_verify_seal_batch): mixes (n, 32), difficulties (n, 32)
    big-endian.  Returns status (n,) uint8: ST_OK, ST_INVALID_DIFFICULTY, ST_INVALID_MIX_DIGEST, ST_INVALID_POW."""
    h, nn = _ethash_rows(hashes, nonces)
    num = np.ascontiguousarray(numbers, np.uint64).reshape(-1)
    mix = _rows32(mixes)
    dif = _rows32(difficulties)
    n = h.shape[0]
    if num.shape[0] != n or mix.shape[0] != n or dif.shape[0] != n:
        raise ValueError("ethash: one block number, mix digest and difficulty per item")
    st = np.zeros(n, np.uint8)
    check(_lib.load().gsv_ethash_verify_seal_batch(self._h, _ptr(num), _ptr(h), _ptr(nn), _ptr(mix), _ptr(dif), n,
                                                   int(bool(test_mode)), _ptr(st)))
    return st


def _ethash_cache_bytes(cache_t) -> int:
    if not cache_t.is_contiguous():
        raise ValueError("ethash: the cache is a contiguous tensor of gsv_ethash_make_cache's bytes")
    return cache_t.numel() * cache_t.element_size()


def _ethash_dataset_items_dev(self, cache_t, first: int, count: int, out_t, stream=None):
    """torch CUDA tensors: cache_t the verification cache's bytes (16-byte aligned), out_t (count, 64) uint8.
    Dataset items [first, first + count).  Only enqueues on `stream`: one launch, no allocation."""
    if out_t is not None and (not out_t.is_contiguous() or out_t.numel() * out_t.element_size() < 64 * int(count)):
        raise ValueError("ethash: out_t holds count rows of 64 bytes")
    check(_lib.load().gsv_ethash_dataset_items_dev(self._h, _tptr(cache_t), _ethash_cache_bytes(cache_t), int(first),
                                                   int(count), _tptr(out_t), _sp(stream)))


def _ethash_light_batch_dev(self, cache_t, dataset_bytes: int, hash_t, nonce_t, mix_t, result_t, stream=None, n=None):
    """torch CUDA tensors: hash_t n rows of 32 bytes (4-byte aligned), nonce_t n int64 / uint64 values (the
    nonce as a number), mix_t and result_t n rows of 32 bytes (any alignment).  Only enqueues on `stream`."""
    n = int(nonce_t.numel()) if n is None else int(n)
    check(_lib.load().gsv_ethash_light_batch_dev(self._h, _tptr(cache_t), _ethash_cache_bytes(cache_t),
                                                 int(dataset_bytes), _tptr(hash_t), _tptr(nonce_t), n, _tptr(mix_t),
                                                 _tptr(result_t), _sp(stream)))


def _ethash_verify_seal_batch_dev(self, cache_t, dataset_bytes: int, hash_t, nonce_t, mix_t, difficulty_t, status_t,
                                  stream=None, n=None):
    """As ethash_light_batch_dev, with the headers' mix digests and 32-byte big-endian difficulties in and one
    status byte per item out."""
    n = int(nonce_t.numel()) if n is None else int(n)
    check(_lib.load().gsv_ethash_verify_seal_batch_dev(self._h, _tptr(cache_t), _ethash_cache_bytes(cache_t),
                                                       int(dataset_bytes), _tptr(hash_t), _tptr(nonce_t), _tptr(mix_t),
                                                       _tptr(difficulty_t), n, _tptr(status_t), _sp(stream)))


def _ethash_caches(self) -> int:
    """epoch caches the context holds for the ethash host forms (at most _lib.ETHASH_MAX_CACHES)"""
    cnt = ctypes.c_size_t()
    check(_lib.load().gsv_ctx_ethash_caches(self._h, ctypes.byref(cnt)))
    return cnt.value


def _ethash_dataset_bytes(dataset_t) -> int:
    if not dataset_t.is_contiguous():
        raise ValueError("ethash: the dataset is a contiguous tensor of its bytes")
    return dataset_t.numel() * dataset_t.element_size()


def _ethash_full_batch_dev(self, dataset_t, hash_t, nonce_t, mix_t, result_t, stream=None, n=None):
    """hashimotoFull over torch CUDA tensors: dataset_t the dataset's bytes (128-byte aligned; its size is the
    tensor's), the rest as ethash_light_batch_dev.  Only enqueues on `stream`: one launch."""
    n = int(nonce_t.numel()) if n is None else int(n)
    check(_lib.load().gsv_ethash_full_batch_dev(self._h, _tptr(dataset_t), _ethash_dataset_bytes(dataset_t),
                                                _tptr(hash_t), _tptr(nonce_t), n, _tptr(mix_t), _tptr(result_t),
                                                _sp(stream)))


def _ethash_verify_seal_full_batch_dev(self, dataset_t, hash_t, nonce_t, mix_t, difficulty_t, status_t, stream=None,
                                       n=None):
    """As ethash_verify_seal_batch_dev, over the dataset."""
    n = int(nonce_t.numel()) if n is None else int(n)
    check(_lib.load().gsv_ethash_verify_seal_full_batch_dev(self._h, _tptr(dataset_t),
                                                            _ethash_dataset_bytes(dataset_t), _tptr(hash_t),
                                                            _tptr(nonce_t), _tptr(mix_t), _tptr(difficulty_t), n,
                                                            _tptr(status_t), _sp(stream)))


def _ethash_search_dev(self, dataset_t, hash_t, difficulty_t, start_t, span: int, offset_t, nonce_out_t, mix_t,
                       result_t, found_t, stream=None, n=None):
    """The nonce search over torch CUDA tensors (gsv.h gsv_ethash_search_dev): header h tries start_t[h] + k for
    k < span; offset_t (n int32 / uint32) gets the smallest winning k or 0xFFFFFFFF, nonce_out_t (n int64 /
    uint64), mix_t / result_t (n rows of 32 bytes) and found_t (n bytes) the winner's.  Only enqueues on
    `stream`: a memset, the search launch and the finish launch."""
    n = int(start_t.numel()) if n is None else int(n)
    check(_lib.load().gsv_ethash_search_dev(self._h, _tptr(dataset_t), _ethash_dataset_bytes(dataset_t),
                                            _tptr(hash_t), _tptr(difficulty_t), _tptr(start_t), n, int(span),
                                            _tptr(offset_t), _tptr(nonce_out_t), _tptr(mix_t), _tptr(result_t),
                                            _tptr(found_t), _sp(stream)))


def _ethash_full_batch(self, numbers, hashes, nonces, test_mode=False):
    """hashimotoFull per (block number, hash without nonce, nonce) (gsv.h gsv_ethash_full_batch): as
    ethash_light_batch, over the epochs' datasets, which the context generates on the device and keeps."""
    h, nn = _ethash_rows(hashes, nonces)
    num = np.ascontiguousarray(numbers, np.uint64).reshape(-1)
    n = h.shape[0]
    if num.shape[0] != n:
        raise ValueError("ethash: one block number per item")
    mix = np.zeros((n, 32), np.uint8)
    res = np.zeros((n, 32), np.uint8)
    check(_lib.load().gsv_ethash_full_batch(self._h, _ptr(num), int(bool(test_mode)), _ptr(h), _ptr(nn), n, _ptr(mix),
                                            _ptr(res)))
    return mix, res


def _ethash_seal_batch(self, numbers, hashes, difficulties, start_nonces, max_attempts: int, test_mode=False):
    """The sealer per header (gsv.h gsv_ethash_seal_batch): difficulties (n, 32) big-endian.  Returns (nonces
    (n,) uint64, mix digests (n, 32), status (n,) uint8: ST_OK, ST_INVALID_DIFFICULTY or ST_NONCE_NOT_FOUND)."""
    h, st0 = _ethash_rows(hashes, start_nonces)
    num = np.ascontiguousarray(numbers, np.uint64).reshape(-1)
    dif = _rows32(difficulties)
    n = h.shape[0]
    if num.shape[0] != n or dif.shape[0] != n:
        raise ValueError("ethash: one block number and difficulty per item")
    nonce = np.zeros(n, np.uint64)
    mix = np.zeros((n, 32), np.uint8)
    st = np.zeros(n, np.uint8)
    check(_lib.load().gsv_ethash_seal_batch(self._h, _ptr(num), int(bool(test_mode)), _ptr(h), _ptr(dif), _ptr(st0), n,
                                            int(max_attempts), _ptr(nonce), _ptr(mix), _ptr(st)))
    return nonce, mix, st


def _ethash_datasets(self) -> int:
    """epoch datasets the context holds for the ethash full and seal forms (at most _lib.ETHASH_MAX_DATASETS)"""
    cnt = ctypes.c_size_t()
    check(_lib.load().gsv_ctx_ethash_datasets(self._h, ctypes.byref(cnt)))
    return cnt.value


def _config_ref(config):
    """a gsv.params.ChainConfig (or a _lib.ChainConfigStruct) as the pointer the C ABI takes"""
    st = config if isinstance(config, _lib.ChainConfigStruct) else config.as_struct()
    return st, ctypes.cast(ctypes.pointer(st), ctypes.c_void_p)


def _block_header_hash_batch(self, headers):
    """Header.Hash() and Header.HashNoNonce() of RLP-encoded headers (gsv.h gsv_block_header_hash_batch).  Returns
    (hashes (n, 32), hashes without nonce (n, 32), status (n,): ST_OK, ST_BAD_RLP or ST_HEADER_TOO_WIDE)."""
    headers = [bytes(h) for h in headers]
    n = len(headers)
    flat, off = _pack(headers)
    h = np.zeros((n, 32), np.uint8)
    hnn = np.zeros((n, 32), np.uint8)
    st = np.zeros(n, np.uint8)
    check(_lib.load().gsv_block_header_hash_batch(self._h, _ptr(flat), _ptr(off), n, _ptr(h), _ptr(hnn), _ptr(st)))
    return h, hnn, st


def _calc_difficulty_batch(self, config, times, parents):
    """CalcDifficulty(config, times[i], parents[i]) over RLP-encoded parents (gsv.h gsv_calc_difficulty_batch).
    Returns (difficulties (n, 32) big-endian, status (n,))."""
    parents = [bytes(h) for h in parents]
    n = len(parents)
    t = np.ascontiguousarray(times, np.uint64).reshape(-1)
    if t.shape[0] != n:
        raise ValueError("headers: one time per parent")
    flat, off = _pack(parents)
    out = np.zeros((n, 32), np.uint8)
    st = np.zeros(n, np.uint8)
    keep, cfg = _config_ref(config)
    check(_lib.load().gsv_calc_difficulty_batch(self._h, cfg, _ptr(t), _ptr(flat), _ptr(off), n, _ptr(out), _ptr(st)))
    return out, st


def _ethash_verify_headers_batch(self, config, headers, seals=None, parent=None, now=0, test_mode=False,
                                 want_hash=False, want_expected=False):
    """Ethash.VerifyHeaders over RLP-encoded headers (gsv.h gsv_ethash_verify_headers_batch): status (n,) uint8, or
    (status, hashes or None, expected difficulties or None) when one of the two is asked for."""
    headers = [bytes(h) for h in headers]
    n = len(headers)
    flat, off = _pack(headers)
    par = _np_u8(parent) if parent else None
    sl = None
    if seals is not None:
        sl = np.ascontiguousarray(np.asarray(seals, bool).astype(np.uint8)).reshape(-1)
        if sl.shape[0] != n:
            raise ValueError("headers: one seal flag per header")
    st = np.zeros(n, np.uint8)
    h = np.zeros((n, 32), np.uint8) if want_hash else None
    want = np.zeros((n, 32), np.uint8) if want_expected else None
    keep, cfg = _config_ref(config)
    check(_lib.load().gsv_ethash_verify_headers_batch(self._h, cfg, _ptr(flat), _ptr(off), n, _ptr(par),
                                                      0 if par is None else par.size, _ptr(sl), int(now),
                                                      int(bool(test_mode)), _ptr(st), _ptr(h), _ptr(want)))
    return (st, h, want) if (want_hash or want_expected) else st


def block_header_work_bytes(n: int) -> int:
    """gsv_block_header_work_bytes: the work area of block_header_rules_dev"""
    return int(_lib.load().gsv_block_header_work_bytes(int(n)))


def _block_header_rules_dev(self, config, rlp_t, off_t, n: int, parent_t, now: int, work_t, hnn_t, nonce_t, mix_t,
                            difficulty_t, pre_t, post_t, hash_t=None, number_t=None, expected_t=None, stream=None):
    """Decode + rules over torch CUDA tensors (gsv.h gsv_block_header_rules_dev): rlp_t the headers' bytes, off_t
    n + 1 int64 offsets, parent_t the parent's RLP or None.  Writes what ethash_verify_seal_batch_dev takes (hnn_t,
    nonce_t, mix_t, difficulty_t) and the pre- and post-seal statuses.  Only enqueues on `stream`: two launches."""
    keep, cfg = _config_ref(config)
    plen = 0 if parent_t is None else int(parent_t.numel())
    check(_lib.load().gsv_block_header_rules_dev(self._h, cfg, _tptr(rlp_t), _tptr(off_t), int(n), _tptr(parent_t),
                                                 plen, int(now), _tptr(work_t), _tptr(hnn_t), _tptr(nonce_t),
                                                 _tptr(mix_t), _tptr(difficulty_t), _tptr(pre_t), _tptr(post_t),
                                                 _tptr(hash_t), _tptr(number_t), _tptr(expected_t), _sp(stream)))


def _block_header_merge_dev(self, pre_t, seal_t, seals_t, post_t, status_t, n=None, stream=None):
    """status = pre, else the seal's where asked for, else post (gsv.h gsv_block_header_merge_dev): one launch"""
    n = int(pre_t.numel()) if n is None else int(n)
    check(_lib.load().gsv_block_header_merge_dev(self._h, _tptr(pre_t), _tptr(seal_t), _tptr(seals_t), _tptr(post_t),
                                                 n, _tptr(status_t), _sp(stream)))


def _bloom9_batch(self, items) -> np.ndarray:
    """bloom9's three bit numbers of each byte string (gsv.h gsv_bloom9_batch): (n, 3) uint16"""
    items = [bytes(x) for x in items]
    n = len(items)
    flat, off = _pack(items)
    out = np.zeros((n, 3), np.uint16)
    check(_lib.load().gsv_bloom9_batch(self._h, _ptr(flat), _ptr(off), n, _ptr(out)))
    return out


def _bloom9_batch_dev(self, data_t, off_t, idx_t, n=None, stream=None):
    """data_t: torch uint8 CUDA tensor; off_t: n + 1 int64 offsets on the device; idx_t: (n, 3) int16 rows"""
    n = int(off_t.numel()) - 1 if n is None else int(n)
    check(_lib.load().gsv_bloom9_batch_dev(self._h, _tptr(data_t), _tptr(off_t), n, _tptr(idx_t), _sp(stream)))


def _receipt_tables(lists):
    """lists of receipt RLPs -> (flat uint8, voff uint64[receipts + 1], list_off uint64[lists + 1])"""
    items = [bytes(x) for lst in lists for x in lst]
    flat, voff = _pack(items)
    list_off = np.zeros(len(lists) + 1, np.uint64)
    list_off[1:] = np.cumsum([len(lst) for lst in lists])
    return flat, voff, list_off


def _rows_or_none(a, n, width, what):
    if a is None:
        return None
    a = np.ascontiguousarray(np.frombuffer(b"".join(bytes(x) for x in a), np.uint8) if isinstance(a, (list, tuple))
                             else a, np.uint8).reshape(-1)
    if a.size != n * width:
        raise ValueError(f"receipts: one {what} of {width} bytes per list")
    return a


def _receipts_verify_batch(self, lists, want_bloom=None, want_root=None, want_gas=None):
    """The receipt half of ValidateState over lists of RLP-encoded receipts (gsv.h gsv_receipts_verify_batch).
    want_bloom (n x 256 bytes), want_root (n x 32), want_gas (n integers): each None skips that compare.  Returns
    (status (n,), receipt status (receipts,), blooms (n, 256), roots (n, 32), gas used (n,) uint64)."""
    lists = [list(lst) for lst in lists]
    n = len(lists)
    flat, voff, list_off = _receipt_tables(lists)
    nr = int(list_off[-1])
    wb = _rows_or_none(want_bloom, n, 256, "bloom")
    wr = _rows_or_none(want_root, n, 32, "receipt hash")
    wg = None
    if want_gas is not None:
        wg = np.ascontiguousarray(want_gas, np.uint64).reshape(-1)
        if wg.shape[0] != n:
            raise ValueError("receipts: one gas-used value per list")
    st = np.zeros(n, np.uint8)
    rst = np.zeros(nr, np.uint8)
    bloom = np.zeros((n, 256), np.uint8)
    root = np.zeros((n, 32), np.uint8)
    gas = np.zeros(n, np.uint64)
    check(_lib.load().gsv_receipts_verify_batch(self._h, _ptr(flat), _ptr(voff), _ptr(list_off), n, _ptr(wb), _ptr(wr),
                                                _ptr(wg), _ptr(rst), _ptr(bloom), _ptr(root), _ptr(gas), _ptr(st)))
    return st, rst, bloom, root, gas


def receipts_work_bytes(n_receipts: int, vals_bytes: int) -> int:
    """gsv_receipts_work_bytes: the work area of receipts_bloom_dev (0: past the call's bounds)"""
    return int(_lib.load().gsv_receipts_work_bytes(int(n_receipts), int(vals_bytes)))


def _receipts_bloom_dev(self, vals_t, voff_t, n_receipts: int, list_off_t, n_lists: int, vals_bytes: int, work_t,
                        receipt_status_t, receipt_bloom_t, list_bloom_t, gas_used_t, list_status_t, stream=None):
    """Decode + blooms over torch CUDA tensors (gsv.h gsv_receipts_bloom_dev): both offset tables on the device.
    Only enqueues on `stream`: memset nodes and three launches."""
    check(_lib.load().gsv_receipts_bloom_dev(self._h, _tptr(vals_t), _tptr(voff_t), int(n_receipts), _tptr(list_off_t),
                                             int(n_lists), int(vals_bytes), _tptr(work_t), _tptr(receipt_status_t),
                                             _tptr(receipt_bloom_t), _tptr(list_bloom_t), _tptr(gas_used_t),
                                             _tptr(list_status_t), _sp(stream)))


def _receipts_check_dev(self, list_status_t, list_bloom_t, root_t, gas_used_t, want_bloom_t, want_root_t, want_gas_t,
                        n_lists: int, status_t, stream=None):
    """gas used, bloom and receipt root against the header's (gsv.h gsv_receipts_check_dev): one launch"""
    check(_lib.load().gsv_receipts_check_dev(self._h, _tptr(list_status_t), _tptr(list_bloom_t), _tptr(root_t),
                                             _tptr(gas_used_t), _tptr(want_bloom_t), _tptr(want_root_t),
                                             _tptr(want_gas_t), int(n_lists), _tptr(status_t), _sp(stream)))


# ------------------------------------------------------------------ bloombits: generator, codec, matcher, bloomFilter
def _bloombits_generate_batch(self, blooms, section_size: int) -> np.ndarray:
    """The bit vectors of whole sections (gsv.h gsv_bloombits_generate_batch).  blooms: (n_sections * section_size,
    256) bytes; returns (n_sections, 2048, section_size // 8) uint8."""
    rows = np.ascontiguousarray(blooms, np.uint8).reshape(-1, 256)
    s = int(section_size)
    if s <= 0 or rows.shape[0] % s:
        raise ValueError("bloombits: a whole number of sections of section_size blooms")
    n = rows.shape[0] // s
    out = np.zeros((n, _lib.BLOOM_BITS, s // 8), np.uint8)
    check(_lib.load().gsv_bloombits_generate_batch(self._h, _ptr(rows), n, s, _ptr(out)))
    return out


def _bloombits_generate_dev(self, blooms_t, n_sections: int, section_size: int, bits_t, stream=None):
    """blooms_t: n_sections * section_size rows of 256 bytes; bits_t: the table; torch uint8 CUDA tensors"""
    check(_lib.load().gsv_bloombits_generate_dev(self._h, _tptr(blooms_t), int(n_sections), int(section_size),
                                                 _tptr(bits_t), _sp(stream)))


def _bitset_compress_batch(self, vectors):
    """bitutil.CompressBytes of n vectors of one length (gsv.h gsv_bitset_compress_batch): a list of bytes"""
    rows = np.ascontiguousarray(vectors, np.uint8)
    rows = rows.reshape(rows.shape[0], -1) if rows.ndim else rows.reshape(0, 1)
    n, length = rows.shape
    out = np.zeros(max(n * length, 1), np.uint8)
    off = np.zeros(n + 1, np.uint64)
    check(_lib.load().gsv_bitset_compress_batch(self._h, _ptr(rows), n, length, _ptr(out), _ptr(off)))
    return [out[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)]


def _bitset_compress_batch_dev(self, in_t, n: int, length: int, slots_t, len_t, stream=None):
    """in_t, slots_t: n rows of `length` bytes; len_t: n int32; torch CUDA tensors"""
    check(_lib.load().gsv_bitset_compress_batch_dev(self._h, _tptr(in_t), int(n), int(length), _tptr(slots_t),
                                                    _tptr(len_t), _sp(stream)))


def _bitset_decompress_batch(self, items, target: int):
    """bitutil.DecompressBytes(item, target) of each byte string (gsv.h gsv_bitset_decompress_batch): (rows
    (n, target) uint8, status (n,) uint8)"""
    items = [bytes(x) for x in items]
    n = len(items)
    flat, off = _pack(items)
    out = np.zeros((n, int(target)), np.uint8)
    st = np.zeros(n, np.uint8)
    check(_lib.load().gsv_bitset_decompress_batch(self._h, _ptr(flat), _ptr(off), n, int(target), _ptr(out), _ptr(st)))
    return out, st


def _bitset_decompress_batch_dev(self, data_t, off_t, n: int, length: int, out_t, status_t, stream=None):
    check(_lib.load().gsv_bitset_decompress_batch_dev(self._h, _tptr(data_t), _tptr(off_t), int(n), int(length),
                                                      _tptr(out_t), _tptr(status_t), _sp(stream)))


def _filter_tables(queries):
    """queries: per query a list of rules, a rule a list of clauses (bytes, or None for a nil clause), or None for a nil
    rule -> (flat, clause_off, nil, rule_off, query_off) as the host forms take the filter"""
    clauses, nil, rule_off, query_off = [], [], [0], [0]
    for rules in queries:
        for rule in rules or []:
            for cl in rule or []:
                nil.append(1 if cl is None else 0)
                clauses.append(b"" if cl is None else bytes(cl))
            rule_off.append(len(clauses))
        query_off.append(len(rule_off) - 1)
    flat, clause_off = _pack(clauses)
    return (flat, clause_off, np.array(nil + [0], np.uint8), np.array(rule_off, np.uint64),
            np.array(query_off, np.uint64))


def _bloombits_match_batch(self, table, section_size: int, first_section: int, queries, begin, end, capacity=None):
    """Many queries over one table (gsv.h gsv_bloombits_match_batch).  table: (n_sections, 2048, section_size // 8)
    uint8; queries as _filter_tables takes them; begin / end: one block range per query, both ends included.
    Returns a list of uint64 arrays, one per query.  capacity None: the call is repeated with the true total when
    the first guess was short."""
    bits = np.ascontiguousarray(table, np.uint8)
    s = int(section_size)
    n_sections = bits.size // (_lib.BLOOM_BITS * (s // 8)) if s >= 8 else 0
    nq = len(queries)
    flat, coff, nil, roff, qoff = _filter_tables(queries)
    b = np.ascontiguousarray(begin, np.uint64).reshape(-1)
    e = np.ascontiguousarray(end, np.uint64).reshape(-1)
    if b.shape[0] != nq or e.shape[0] != nq:
        raise ValueError("bloombits: one [begin, end] per query")
    cap = 4096 * max(nq, 1) if capacity is None else int(capacity)
    while True:
        block_off = np.zeros(nq + 1, np.uint64)
        blocks = np.zeros(max(cap, 1), np.uint64)
        check(_lib.load().gsv_bloombits_match_batch(self._h, _ptr(bits), s, int(first_section), n_sections, _ptr(flat),
                                                    _ptr(coff), _ptr(nil), _ptr(roff), _ptr(qoff), nq, _ptr(b), _ptr(e),
                                                    _ptr(block_off), _ptr(blocks), cap))
        total = int(block_off[-1])
        if total <= cap or capacity is not None:
            break
        cap = total
    return [blocks[int(block_off[q]):min(int(block_off[q + 1]), cap)].copy() for q in range(nq)]


def _bloombits_match_dev(self, bits_t, section_size: int, first_section: int, n_sections: int, clauses_t, n_clauses: int,
                         rule_off_t, n_rules: int, query_off_t, n_queries: int, begin_t, end_t, match_t, count_t,
                         stream=None):
    """The match bitsets and counts over torch CUDA tensors (gsv.h gsv_bloombits_match_dev): clauses_t (n, 3) int16 as
    bloom9_batch_dev writes them, the two tables int32, the ranges int64"""
    check(_lib.load().gsv_bloombits_match_dev(self._h, _tptr(bits_t), int(section_size), int(first_section),
                                              int(n_sections), _tptr(clauses_t), int(n_clauses), _tptr(rule_off_t),
                                              int(n_rules), _tptr(query_off_t), int(n_queries), _tptr(begin_t),
                                              _tptr(end_t), _tptr(match_t), _tptr(count_t), _sp(stream)))


def _bloombits_blocks_dev(self, match_t, count_t, section_size: int, first_section: int, n_sections: int, n_queries: int,
                          block_off_t, blocks_t, capacity: int, stream=None):
    """The match bitsets as block numbers (gsv.h gsv_bloombits_blocks_dev): block_off_t n_queries + 1 int64, blocks_t
    `capacity` int64"""
    check(_lib.load().gsv_bloombits_blocks_dev(self._h, _tptr(match_t), _tptr(count_t), int(section_size),
                                               int(first_section), int(n_sections), int(n_queries), _tptr(block_off_t),
                                               _tptr(blocks_t), int(capacity), _sp(stream)))


def _bloom_filter_batch(self, blooms, queries) -> np.ndarray:
    """bloomFilter of every bloom under every query (gsv.h gsv_bloom_filter_batch): (n_queries, n_blooms) bool"""
    rows = np.ascontiguousarray(blooms, np.uint8).reshape(-1, 256)
    nq = len(queries)
    flat, coff, nil, roff, qoff = _filter_tables(queries)
    out = np.zeros((nq, rows.shape[0]), np.uint8)
    check(_lib.load().gsv_bloom_filter_batch(self._h, _ptr(rows), rows.shape[0], _ptr(flat), _ptr(coff), _ptr(nil),
                                             _ptr(roff), _ptr(qoff), nq, _ptr(out)))
    return out.astype(bool)


def _bloom_filter_dev(self, blooms_t, n_blooms: int, clauses_t, n_clauses: int, rule_off_t, n_rules: int, query_off_t,
                      n_queries: int, out_t, stream=None):
    check(_lib.load().gsv_bloom_filter_dev(self._h, _tptr(blooms_t), int(n_blooms), _tptr(clauses_t), int(n_clauses),
                                           _tptr(rule_off_t), int(n_rules), _tptr(query_off_t), int(n_queries),
                                           _tptr(out_t), _sp(stream)))


def _arena_read(self, off, n):
    """Test hook (gsv.h gsv_ctx_arena_read): n bytes of the staging arena from `off`, as they are now."""
    out = np.zeros(n, np.uint8)
    check(_lib.load().gsv_ctx_arena_read(self._h, off, n, _ptr(out)))
    return out


def _prepared_shapes(self):
    cnt = ctypes.c_size_t()
    nb = ctypes.c_size_t()
    check(_lib.load().gsv_ctx_prepared_shapes(self._h, ctypes.byref(cnt), ctypes.byref(nb)))
    return cnt.value, nb.value


Context.ecrecover_precompile_batch = _ecrecover_precompile_batch
Context.ecrecover_precompile_batch_dev = _ecrecover_precompile_batch_dev
Context.ecdsa_verify_batch = _ecdsa_verify_batch
Context.ecdsa_verify_batch_dev = _ecdsa_verify_batch_dev
Context.pubkey_parse_batch = _pubkey_parse_batch
Context.pubkey_parse_batch_dev = _pubkey_parse_batch_dev
Context.ecdsa_sign_batch = _ecdsa_sign_batch
Context.ecdsa_sign_batch_dev = _ecdsa_sign_batch_dev
Context.pubkey_create_batch = _pubkey_create_batch
Context.pubkey_create_batch_dev = _pubkey_create_batch_dev
Context.tx_sign_batch = _tx_sign_batch
Context.tx_sign_batch_dev = _tx_sign_batch_dev
Context.secp256k1_scalar_mul_batch = _secp256k1_scalar_mul_batch
Context.secp256k1_scalar_mul_batch_dev = _secp256k1_scalar_mul_batch_dev
Context.ecdh_batch = _ecdh_batch
Context.ecdh_batch_dev = _ecdh_batch_dev
Context.ecies_decrypt_batch = _ecies_decrypt_batch
Context.ecies_encrypt_batch = _ecies_encrypt_batch
Context.ecies_decrypt_batch_dev = _ecies_decrypt_batch_dev
Context.ecies_encrypt_batch_dev = _ecies_encrypt_batch_dev
Context.ethash_light_batch = _ethash_light_batch
Context.ethash_verify_seal_batch = _ethash_verify_seal_batch
Context.ethash_dataset_items_dev = _ethash_dataset_items_dev
Context.ethash_light_batch_dev = _ethash_light_batch_dev
Context.ethash_verify_seal_batch_dev = _ethash_verify_seal_batch_dev
Context.ethash_caches = _ethash_caches
Context.ethash_full_batch = _ethash_full_batch
Context.ethash_seal_batch = _ethash_seal_batch
Context.ethash_full_batch_dev = _ethash_full_batch_dev
Context.ethash_verify_seal_full_batch_dev = _ethash_verify_seal_full_batch_dev
Context.ethash_search_dev = _ethash_search_dev
Context.ethash_datasets = _ethash_datasets
Context.block_header_hash_batch = _block_header_hash_batch
Context.calc_difficulty_batch = _calc_difficulty_batch
Context.ethash_verify_headers_batch = _ethash_verify_headers_batch
Context.block_header_rules_dev = _block_header_rules_dev
Context.block_header_merge_dev = _block_header_merge_dev
Context.bloom9_batch = _bloom9_batch
Context.bloom9_batch_dev = _bloom9_batch_dev
Context.receipts_verify_batch = _receipts_verify_batch
Context.receipts_bloom_dev = _receipts_bloom_dev
Context.receipts_check_dev = _receipts_check_dev
Context.bloombits_generate_batch = _bloombits_generate_batch
Context.bloombits_generate_dev = _bloombits_generate_dev
Context.bitset_compress_batch = _bitset_compress_batch
Context.bitset_compress_batch_dev = _bitset_compress_batch_dev
Context.bitset_decompress_batch = _bitset_decompress_batch
Context.bitset_decompress_batch_dev = _bitset_decompress_batch_dev
Context.bloombits_match_batch = _bloombits_match_batch
Context.bloombits_match_dev = _bloombits_match_dev
Context.bloombits_blocks_dev = _bloombits_blocks_dev
Context.bloom_filter_batch = _bloom_filter_batch
Context.bloom_filter_dev = _bloom_filter_dev
Context.modexp_batch = _modexp_batch
Context.modexp_batch_dev = _modexp_batch_dev
Context._arena_read = _arena_read
Context.prepared_shapes = _prepared_shapes
Context.bn256_add_batch = _bn256_add_batch
Context.bn256_scalar_mul_batch = _bn256_scalar_mul_batch
Context.bn256_add_batch_dev = _bn256_add_batch_dev
Context.bn256_scalar_mul_batch_dev = _bn256_scalar_mul_batch_dev


# ------------------------------------------------------------------ blob codec, createCollation
def _blob_tables(lists):
    """lists of byte strings -> (flat uint8, blob_off uint64[nblobs+1], list_off uint64[n+1])"""
    blobs = [bytes(b) for lst in lists for b in lst]
    flat, blob_off = _pack(blobs)
    list_off = np.zeros(len(lists) + 1, np.uint64)
    list_off[1:] = np.cumsum([len(lst) for lst in lists])
    return flat, blob_off, list_off


def blob_serialized_size(blob_off, list_off) -> np.ndarray:
    """Body offsets (n_lists + 1) of utils.Serialize over these lists (gsv.h gsv_blob_serialized_size):
    host arithmetic, no GPU."""
    blob_off = np.ascontiguousarray(blob_off, np.uint64)
    list_off = np.ascontiguousarray(list_off, np.uint64)
    out = np.zeros(list_off.shape[0], np.uint64)
    check(_lib.load().gsv_blob_serialized_size(_ptr(blob_off), _ptr(list_off), list_off.shape[0] - 1, _ptr(out)))
    return out


def blob_data_layout(off) -> np.ndarray:
    """Data-region offsets (n + 1) of the device-resident Deserialize (gsv.h gsv_blob_data_layout)."""
    off = np.ascontiguousarray(off, np.uint64)
    out = np.zeros(off.shape[0], np.uint64)
    check(_lib.load().gsv_blob_data_layout(_ptr(off), off.shape[0] - 1, _ptr(out)))
    return out


def proposer_body_layout(blob_off, list_off):
    """(body_off (n + 1), status (n,)) of createCollation's bodies (gsv.h gsv_proposer_body_layout): an
    oversized collation has ST_BODY_TOO_LARGE and length 0."""
    blob_off = np.ascontiguousarray(blob_off, np.uint64)
    list_off = np.ascontiguousarray(list_off, np.uint64)
    n = list_off.shape[0] - 1
    out = np.zeros(n + 1, np.uint64)
    st = np.zeros(n, np.uint8)
    check(_lib.load().gsv_proposer_body_layout(_ptr(blob_off), _ptr(list_off), n, _ptr(out), _ptr(st)))
    return out, st


def _blob_serialize_batch(self, lists, skip_evm=None):
    """utils.Serialize of each list of byte strings (gsv.h gsv_blob_serialize_batch): a list of bodies.
    skip_evm: per list, the blobs' flags (None: all false)."""
    n = len(lists)
    if n == 0:
        return []
    flat, blob_off, list_off = _blob_tables(lists)
    sk = None
    if skip_evm is not None:
        sk = np.array([1 if f else 0 for fl in skip_evm for f in fl] + [0], np.uint8)
        if sk.shape[0] - 1 != blob_off.shape[0] - 1:
            raise ValueError("skip_evm and blobs sizes differ")
    body_off = blob_serialized_size(blob_off, list_off)
    out = np.zeros(int(body_off[n]) + 1, np.uint8)
    check(_lib.load().gsv_blob_serialize_batch(self._h, _ptr(flat), _ptr(blob_off), _ptr(sk) if sk is not None else None,
                                               _ptr(list_off), n, _ptr(out), _ptr(body_off)))
    return [out[int(body_off[i]):int(body_off[i + 1])].tobytes() for i in range(n)]


def _blob_serialize_prepare(self, blob_off, list_off):
    blob_off = np.ascontiguousarray(blob_off, np.uint64)
    list_off = np.ascontiguousarray(list_off, np.uint64)
    check(_lib.load().gsv_blob_serialize_prepare(self._h, _ptr(blob_off), _ptr(list_off), list_off.shape[0] - 1))


def _blob_serialize_batch_dev(self, blobs_t, blob_off, list_off, bodies_t, skip_t=None, stream=None, prepare=True):
    """blobs_t / skip_t / bodies_t: torch uint8 CUDA tensors; blob_off, list_off: numpy uint64 (host).
    bodies_t follows blob_serialized_size's layout and is 16-byte aligned."""
    blob_off = np.ascontiguousarray(blob_off, np.uint64)
    list_off = np.ascontiguousarray(list_off, np.uint64)
    if prepare:
        _blob_serialize_prepare(self, blob_off, list_off)
    sp = _sp(stream)
    check(_lib.load().gsv_blob_serialize_batch_dev(self._h, _tptr(blobs_t), _ptr(blob_off), _tptr(skip_t),
                                                   _ptr(list_off), list_off.shape[0] - 1, _tptr(bodies_t), sp))


def _blob_deserialize_batch(self, bodies):
    """utils.Deserialize of each body (gsv.h gsv_blob_deserialize_batch): per body, the list of
    (blob bytes, skip_evm) the reference returns."""
    n = len(bodies)
    if n == 0:
        return []
    flat, off = _pack(bodies)
    chunks = int(sum(len(b) // 32 for b in bodies))
    nb = np.zeros(n, np.uint32)
    boff = np.zeros(chunks + 1, np.uint64)
    sk = np.zeros(chunks + 1, np.uint8)
    data = np.zeros(31 * chunks + 1, np.uint8)
    check(_lib.load().gsv_blob_deserialize_batch(self._h, _ptr(flat), _ptr(off), n, _ptr(nb), _ptr(boff), _ptr(sk),
                                                 _ptr(data)))
    out, k = [], 0
    for i in range(n):
        out.append([(data[int(boff[k + t]):int(boff[k + t + 1])].tobytes(), int(sk[k + t])) for t in range(int(nb[i]))])
        k += int(nb[i])
    return out


def _blob_deserialize_prepare(self, h_off, max_blobs: int):
    h_off = np.ascontiguousarray(h_off, np.uint64)
    check(_lib.load().gsv_blob_deserialize_prepare(self._h, _ptr(h_off), h_off.shape[0] - 1, int(max_blobs)))


def _blob_deserialize_batch_dev(self, bodies_t, h_off, max_blobs, nblobs_t, start_t, len_t, skip_t, data_t=None,
                                stream=None, prepare=True):
    """bodies_t: torch uint8 CUDA; nblobs_t (n,) / start_t, len_t (n, max_blobs) int32-sized; skip_t
    (n, max_blobs) uint8; data_t: uint8, blob_data_layout's regions (None: index only)."""
    h_off = np.ascontiguousarray(h_off, np.uint64)
    if prepare:
        _blob_deserialize_prepare(self, h_off, max_blobs)
    sp = _sp(stream)
    check(_lib.load().gsv_blob_deserialize_batch_dev(self._h, _tptr(bodies_t), _ptr(h_off), h_off.shape[0] - 1,
                                                     int(max_blobs), _tptr(nblobs_t), _tptr(start_t), _tptr(len_t),
                                                     _tptr(skip_t), _tptr(data_t), sp))


def _proposer_create_collations(self, tx_lists, shard_id32, period32, proposer20, seckey32):
    """proposer.createCollation over a batch (gsv.h gsv_proposer_create_collations): tx_lists[i] = the
    encoded transactions of collation i; the other arrays (n, 32) / (n, 20) uint8.  Returns (bodies (list
    of bytes), chunk_root (n,32), hash (n,32), sig (n,65), status (n,)).  The keys' device copy is
    overwritten before the call returns."""
    n = len(tx_lists)
    sid = _np_u8(shard_id32).reshape(n, 32)
    per = _np_u8(period32).reshape(n, 32)
    prop = _np_u8(proposer20).reshape(n, 20)
    keys = _seckey_rows(seckey32)
    if keys.shape[0] != n:
        raise ValueError("tx_lists and keys batch sizes differ")
    root = np.zeros((n, 32), np.uint8)
    h = np.zeros((n, 32), np.uint8)
    sig = np.zeros((n, 65), np.uint8)
    st = np.zeros(n, np.uint8)
    if n == 0:
        return [], root, h, sig, st
    flat, blob_off, list_off = _blob_tables(tx_lists)
    body_off, _ = proposer_body_layout(blob_off, list_off)
    out = np.zeros(int(body_off[n]) + 1, np.uint8)
    check(_lib.load().gsv_proposer_create_collations(self._h, _ptr(flat), _ptr(blob_off), _ptr(list_off), n, _ptr(sid),
                                                     _ptr(per), _ptr(prop), _ptr(keys), _ptr(out), _ptr(body_off),
                                                     _ptr(root), _ptr(h), _ptr(sig), _ptr(st)))
    bodies = [out[int(body_off[i]):int(body_off[i + 1])].tobytes() for i in range(n)]
    return bodies, root, h, sig, st


def _proposer_prepare(self, blob_off, list_off):
    blob_off = np.ascontiguousarray(blob_off, np.uint64)
    list_off = np.ascontiguousarray(list_off, np.uint64)
    check(_lib.load().gsv_proposer_prepare(self._h, _ptr(blob_off), _ptr(list_off), list_off.shape[0] - 1))


def _proposer_create_collations_dev(self, blobs_t, blob_off, list_off, sid_t, per_t, prop_t, key_t, bodies_t, root_t,
                                    hash_t, sig_t, st_t, stream=None, prepare=True):
    """torch uint8 CUDA tensors (blob_off, list_off: numpy uint64 on the host); bodies_t follows
    proposer_body_layout.  Only enqueues on `stream`; key_t is the caller's to wipe."""
    blob_off = np.ascontiguousarray(blob_off, np.uint64)
    list_off = np.ascontiguousarray(list_off, np.uint64)
    if prepare:
        _proposer_prepare(self, blob_off, list_off)
    sp = _sp(stream)
    check(_lib.load().gsv_proposer_create_collations_dev(
        self._h, _tptr(blobs_t), _ptr(blob_off), _ptr(list_off), list_off.shape[0] - 1, _tptr(sid_t), _tptr(per_t),
        _tptr(prop_t), _tptr(key_t), _tptr(bodies_t), _tptr(root_t), _tptr(hash_t), _tptr(sig_t), _tptr(st_t), sp))


Context.blob_serialize_batch = _blob_serialize_batch
Context.blob_serialize_prepare = _blob_serialize_prepare
Context.blob_serialize_batch_dev = _blob_serialize_batch_dev
Context.blob_deserialize_batch = _blob_deserialize_batch
Context.blob_deserialize_prepare = _blob_deserialize_prepare
Context.blob_deserialize_batch_dev = _blob_deserialize_batch_dev
Context.proposer_create_collations = _proposer_create_collations
Context.proposer_prepare = _proposer_prepare
Context.proposer_create_collations_dev = _proposer_create_collations_dev
