"""TEST INFRASTRUCTURE — the collation-header corpus of tests/test_header_cases.py (CPU) and
tests/test_gpu_header.py (GPU), with its expected results from the CPU oracle alone.

Deterministic: one fixed key, fixed seeds, a per-case nonce.  Four families:

  a  every byte length 0..32 of ShardID x every byte length 0..32 of Period x nil bits {0, 1, 2, 3}, each
     validly signed by KEY (4,356 headers: signed RLP of every length 73..189, unsigned 6..123)
  b  the single-byte rule: ShardID, Period in {0x01, 0x7f, 0x80, 0xff}
  c  1,024 random headers, nil bits 0..7; every fourth has two full 32-byte integers and no nil field
     (the benchmark's 189-byte shape)
  d  the status classes of gsv_collation_header_verify_batch, each with and without a ChunkRoot

A nil field's row of the C ABI is filled with 0xA5, not zeros, so a kernel that reads a row it must
ignore shows.  Expected results per case (crypto.Ecrecover's rules, crypto/secp256k1/secp256.go:105-124,
:171-174):

  nil bit 2 set, whatever the sig65 row holds     GSV_ST_INVALID_SIG_LEN, signer zero
  oracle.ecrecover(msg, sig) -> -1                GSV_ST_INVALID_RECID, signer zero
                             ->  0                GSV_ST_RECOVER_FAILED, signer zero
                             ->  1                GSV_ST_OK iff ProposerAddress is set and equals
                                                  Keccak256(pub[1:])[12:], else GSV_ST_PROPOSER_MISMATCH;
                                                  the signer is reported in both
"""
from __future__ import annotations

import random

import numpy as np

KEY = bytes.fromhex("4c0883a69102937d6231471b5dbb6204fe5129617082792ae468d01a3f362318")
SECP_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
FILL = 0xA5
FIRST = (0x01, 0x7f, 0x80, 0xff)  # first byte of a multi-byte integer

# include/gsv.h
ST_OK, ST_INVALID_SIG_LEN, ST_INVALID_RECID, ST_RECOVER_FAILED, ST_PROPOSER_MISMATCH = 0, 2, 3, 4, 10
ALL_STATUSES = {ST_OK, ST_INVALID_SIG_LEN, ST_INVALID_RECID, ST_RECOVER_FAILED, ST_PROPOSER_MISMATCH}


class Case:
    """One header.  shard_id / period: ints; chunk_root / proposer: bytes or None (nil bits 0 / 1);
    sig65: the header's signature, or None (nil bit 2: the sig65 row then holds sig_row, 0xA5 bytes
    unless given).  rlp / unsigned_rlp / hash32 / msg / status / signer: the expected results."""
    __slots__ = ("family", "label", "shard_id", "period", "chunk_root", "proposer", "sig65", "sig_row", "nil",
                 "rlp", "unsigned_rlp", "hash32", "msg", "status", "signer")

    def __init__(self, family, label, shard_id, chunk_root, period, proposer, sig65=None, sig_row=None):
        self.family, self.label = family, label
        self.shard_id, self.period, self.chunk_root, self.proposer = shard_id, period, chunk_root, proposer
        self.sig65 = sig65
        self.sig_row = bytes([FILL]) * 65 if sig_row is None else sig_row
        self.nil = (chunk_root is None) | (proposer is None) << 1 | (sig65 is None) << 2

    def rows(self):
        """(shard_id32, chunk_root32, period32, proposer20, sig65) as the C ABI takes them"""
        return (self.shard_id.to_bytes(32, "big"),
                bytes([FILL]) * 32 if self.chunk_root is None else self.chunk_root,
                self.period.to_bytes(32, "big"),
                bytes([FILL]) * 20 if self.proposer is None else self.proposer,
                self.sig_row if self.sig65 is None else self.sig65)


def pack(cases):
    """-> (sid (n,32), root (n,32), per (n,32), prop (n,20), sig (n,65), nil (n,)) uint8 arrays"""
    cols = list(zip(*(c.rows() for c in cases)))
    out = [np.frombuffer(b"".join(col), np.uint8).reshape(len(cases), -1).copy() for col in cols]
    return (*out, np.array([c.nil for c in cases], np.uint8))


def address(O):
    return O.keccak256(O.secp_pubkey(KEY)[1:])[12:]


_NONCE = [0]


def sign(O, shard_id, chunk_root, period, proposer):
    """[R || S || V] by KEY over the header's hash with the signature empty (proposer.go:77-89)"""
    _NONCE[0] += 1
    msg = O.collation_header_hash(shard_id, chunk_root, period, proposer, None)
    return O.secp_sign(msg, KEY, O.keccak256(b"gsv-header-cases" + _NONCE[0].to_bytes(4, "big")))


def _signed(O, family, label, shard_id, chunk_root, period, proposer):
    return Case(family, label, shard_id, chunk_root, period, proposer,
                sign(O, shard_id, chunk_root, period, proposer))


def _integer(rng, length, first):
    """an integer of exactly `length` bytes; a one-byte one is >= 0x80 (two bytes of RLP: family b has
    the bare bytes), a longer one starts with `first`"""
    if length == 0:
        return 0
    if length == 1:
        return 0x80 | rng.getrandbits(7)
    return int.from_bytes(bytes([first]) + rng.randbytes(length - 1), "big")


def family_a(O):
    rng, addr, out = random.Random(0xA), address(O), []
    for nil in range(4):
        for ls in range(33):
            for lp in range(33):
                i = len(out)
                out.append(_signed(O, "a", f"a: shard_id {ls} B, period {lp} B, nil {nil}",
                                   _integer(rng, ls, FIRST[i % 4]), None if nil & 1 else rng.randbytes(32),
                                   _integer(rng, lp, FIRST[i // 4 % 4]), None if nil & 2 else addr))
    return out


def family_b(O):
    rng, addr = random.Random(0xB), address(O)
    return [_signed(O, "b", f"b: shard_id {s:#04x}, period {p:#04x}", s, rng.randbytes(32), p, addr)
            for s in FIRST for p in FIRST]


def family_c(O):
    rng, out = random.Random(0xC), []
    for i in range(1024):
        bench = i % 4 == 0
        nil = 0 if bench else rng.randrange(8)
        sid, per = (int.from_bytes(rng.randbytes(32 if bench else rng.randrange(33)), "big") for _ in range(2))
        root = None if nil & 1 else rng.randbytes(32)
        prop = None if nil & 2 else rng.randbytes(20)
        label = f"c: random {i}, nil {nil}" + (", benchmark shape" if bench else "")
        out.append(Case("c", label, sid, root, per, prop) if nil & 4 else _signed(O, "c", label, sid, root, per, prop))
    return out


def _flip(b, i):
    return b[:i] + bytes([b[i] ^ 1]) + b[i + 1:]


def family_d(O):
    rng, addr, out = random.Random(0xD), address(O), []
    for nil0 in (0, 1):
        sid, per = int.from_bytes(rng.randbytes(5), "big") | 1 << 39, int.from_bytes(rng.randbytes(3), "big") | 1 << 23
        root = None if nil0 else rng.randbytes(32)

        def with_sig(label, sig, prop=addr):
            out.append(Case("d", f"d: {label}, nil {nil0}", sid, root, per, prop, sig))

        for k in (0, 19):
            out.append(_signed(O, "d", f"d: proposer differs in byte {k}, nil {nil0}", sid, root, per, _flip(addr, k)))
        out.append(_signed(O, "d", f"d: nil proposer, valid signature, nil {nil0 | 2}", sid, root, per, None))
        good = sign(O, sid, root, per, addr)
        msg = O.collation_header_hash(sid, root, per, addr, None)
        assert O.ecrecover(msg, good)[0] == 1
        with_sig("recid 4", good[:64] + b"\x04")
        with_sig("recid 255", good[:64] + b"\xff")
        with_sig("r = 0", bytes(32) + good[32:])
        for _ in range(64):  # about half of all r are no x-coordinate
            bad = _flip(sign(O, sid, root, per, addr), 31)
            if O.ecrecover(msg, bad)[0] == 0:
                break
        else:
            raise AssertionError("no r without a curve point found")
        with_sig("r is no x-coordinate", bad)
        s = SECP_N - int.from_bytes(good[32:64], "big")
        with_sig("high-s twin, recid flipped", good[:32] + s.to_bytes(32, "big") + bytes([good[64] ^ 1]))
        with_sig("recid flipped alone", _flip(good, 64))
        for what, row in (("a valid signature", good), ("zeros", bytes(65)), ("0xA5 bytes", None)):
            out.append(Case("d", f"d: nil signature over {what}, nil {nil0 | 4}", sid, root, per, addr, None, row))
    return out


def expect(O, c):
    """fills the case's expected results in, from the oracle only"""
    f = (c.shard_id, c.chunk_root, c.period, c.proposer)
    c.rlp = O.collation_header_rlp(*f, c.sig65)
    c.unsigned_rlp = O.collation_header_rlp(*f, None)
    c.hash32, c.msg = O.keccak256(c.rlp), O.keccak256(c.unsigned_rlp)
    c.signer = bytes(20)
    if c.nil & 4:
        c.status = ST_INVALID_SIG_LEN
        return
    rc, pub = O.ecrecover(c.msg, c.sig65)
    if rc != 1:
        c.status = ST_INVALID_RECID if rc == -1 else ST_RECOVER_FAILED
        return
    c.signer = O.keccak256(pub[1:])[12:]
    c.status = ST_OK if c.proposer is not None and c.proposer == c.signer else ST_PROPOSER_MISMATCH


_CORPUS = []


def corpus(O):
    """every case of the four families with its expected results (built once per process; read-only)"""
    if not _CORPUS:
        _NONCE[0] = 0
        cases = family_a(O) + family_b(O) + family_c(O) + family_d(O)
        for c in cases:
            expect(O, c)
        _CORPUS.extend(cases)
    return _CORPUS
