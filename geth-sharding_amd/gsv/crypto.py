"""Mirror of the reference's crypto package entry points on the hot path, batched on the GPU.

    Keccak256(*data)            crypto/crypto.go:43-49
    Keccak256Hash(*data)        crypto/crypto.go:53-60
    Ecrecover(hash, sig)        crypto/signature_cgo.go:31-33 -> secp256k1.RecoverPubkey (secp256.go:105-122)
    SigToPub(hash, sig)         crypto/signature_cgo.go:36-44 (returns the 65-byte key here)
    EcrecoverBatch(...)         batch form used by the notary / tx pool hooks
    Keccak256Batch(msgs)        batch form
    Sha256(data) / Sha256Batch(msgs)        crypto/sha256.Sum256, as core/vm/contracts.go:114-117 calls it
    Ripemd160(data) / Ripemd160Batch(msgs)  ripemd160.New().Write(data).Sum(nil), as contracts.go:129-133 does
    Ecrecover precompile        core/vm/contracts.go:70-101 (EcrecoverPrecompile.Run / RunBatch)
    VerifySignature(pub, hash, sig)   crypto/signature_cgo.go:63-68 -> secp256k1.VerifySignature
    VerifySignatureBatch(...)   batch form
    DecompressPubkey(pub33)     crypto/signature_cgo.go:71-77 (returns the 65-byte key here)
    CompressPubkey(pub65)       crypto/signature_cgo.go:80-82
    Sign(hash, prv)             crypto/signature_cgo.go:54-61 -> secp256k1.Sign (secp256.go:70-99)
    SignBatch(hashes, keys)     batch form: per-item status codes
    PubkeyFromSeckey(prv)       secp256k1_ec_pubkey_create, the derivation behind crypto.ToECDSA
    ScalarMult(x, y, k)         crypto/secp256k1/curve.go:221-254 -> secp256k1_ext_scalar_mul
    ScalarBaseMult(k)           crypto/secp256k1/curve.go:257-259
    ScalarMultBatch(...)        batch form: per-item status codes

Errors mirror crypto/secp256k1/secp256.go:54-62 and are raised as exceptions.
"""
from __future__ import annotations

import numpy as np

from . import _lib, default_context


class ErrInvalidMsgLen(ValueError):
    """invalid message length, need 32 bytes"""


class ErrInvalidSignatureLen(ValueError):
    """invalid signature length"""


class ErrInvalidRecoveryID(ValueError):
    """invalid signature recovery id"""


class ErrRecoverFailed(ValueError):
    """recovery failed"""


def Keccak256(*data) -> bytes:
    msg = b"".join(bytes(d) for d in data)
    return bytes(default_context().keccak256_batch([msg])[0])


Keccak256Hash = Keccak256


def Keccak256Batch(msgs, ctx=None) -> np.ndarray:
    return (ctx or default_context()).keccak256_batch(list(msgs))


def Sha256Batch(msgs, ctx=None) -> np.ndarray:
    """(n, 32) uint8: the SHA-256 digest of each message"""
    return (ctx or default_context()).sha256_batch([bytes(m) for m in msgs])


def Sha256(data: bytes, ctx=None) -> bytes:
    return bytes(Sha256Batch([data], ctx)[0])


def Ripemd160Batch(msgs, ctx=None) -> np.ndarray:
    """(n, 20) uint8: the RIPEMD-160 digest of each message (the library's rows without their 12 zero bytes)"""
    return (ctx or default_context()).ripemd160_batch([bytes(m) for m in msgs])[:, 12:]


def Ripemd160(data: bytes, ctx=None) -> bytes:
    return bytes(Ripemd160Batch([data], ctx)[0])


def _check_lengths(msg: bytes, sig: bytes):
    # crypto/secp256k1/secp256.go:106-111 + checkSignature :171-178
    if len(msg) != 32:
        raise ErrInvalidMsgLen("invalid message length, need 32 bytes")
    if len(sig) != 65:
        raise ErrInvalidSignatureLen("invalid signature length")
    if sig[64] >= 4:
        raise ErrInvalidRecoveryID("invalid signature recovery id")


def Ecrecover(hash: bytes, sig: bytes) -> bytes:
    """Returns the uncompressed public key (65 bytes) that created the signature."""
    hash, sig = bytes(hash), bytes(sig)
    _check_lengths(hash, sig)
    pub, _, st = default_context().ecrecover_batch(np.frombuffer(hash, np.uint8)[None],
                                                   np.frombuffer(sig, np.uint8)[None])
    if st[0] != _lib.ST_OK:
        raise ErrRecoverFailed("recovery failed")
    return bytes(pub[0])


SigToPub = Ecrecover


def EcrecoverBatch(hashes, sigs, want_pub=True, want_addr=False, ctx=None):
    """Batch ecrecover: per-item status codes (GSV_ST_*) instead of exceptions."""
    return (ctx or default_context()).ecrecover_batch(hashes, sigs, want_pub=want_pub,
                                                      want_addr=want_addr)


class ErrInvalidPubkey(ValueError):
    """invalid public key"""


def VerifySignature(pubkey: bytes, hash: bytes, sig: bytes, ctx=None) -> bool:
    """crypto/signature_cgo.go:63-68 -> secp256k1.VerifySignature (secp256.go:124-134): whether `sig`
    ([R || S], 64 bytes, no recovery id) is a valid lower-s signature of `hash` by `pubkey` (33 or 65
    bytes).  The three length rules come first and need no GPU."""
    pubkey, hash, sig = bytes(pubkey), bytes(hash), bytes(sig)
    if len(hash) != 32 or len(sig) != 64 or len(pubkey) == 0:
        return False
    ok = (ctx or default_context()).ecdsa_verify_batch(np.frombuffer(hash, np.uint8)[None],
                                                       np.frombuffer(sig, np.uint8)[None], [pubkey])
    return bool(ok[0])


def VerifySignatureBatch(pubkeys, hashes, sigs, ctx=None) -> np.ndarray:
    """Batch VerifySignature: a bool per item.  An item with a hash that is not 32 bytes, a signature
    that is not 64 bytes or an empty key is False, as VerifySignature makes it; the rest go to the GPU in
    one call."""
    pubkeys = [bytes(k) for k in pubkeys]
    hashes = [bytes(h) for h in hashes]
    sigs = [bytes(s) for s in sigs]
    n = len(pubkeys)
    if len(hashes) != n or len(sigs) != n:
        raise ValueError("pubkeys, hashes and sigs batch sizes differ")
    out = np.zeros(n, bool)
    idx = [i for i in range(n) if len(hashes[i]) == 32 and len(sigs[i]) == 64 and len(pubkeys[i]) != 0]
    if idx:
        msg = np.frombuffer(b"".join(hashes[i] for i in idx), np.uint8).reshape(-1, 32)
        sg = np.frombuffer(b"".join(sigs[i] for i in idx), np.uint8).reshape(-1, 64)
        ok = (ctx or default_context()).ecdsa_verify_batch(msg, sg, [pubkeys[i] for i in idx])
        out[idx] = ok != 0
    return out


def DecompressPubkey(pubkey: bytes, ctx=None) -> bytes:
    """crypto/signature_cgo.go:71-77: the 65-byte uncompressed form of a 33-byte compressed key."""
    pubkey = bytes(pubkey)
    if len(pubkey) != 33:  # secp256k1.DecompressPubkey returns (nil, nil) before any parsing
        raise ErrInvalidPubkey("invalid public key")
    pub, ok = (ctx or default_context()).pubkey_parse_batch([pubkey])
    if not ok[0]:
        raise ErrInvalidPubkey("invalid public key")
    return bytes(pub[0])


def CompressPubkey(pubkey: bytes, ctx=None) -> bytes:
    """crypto/signature_cgo.go:80-82: 02 | 03 followed by X.  The reference panics on a key that does not
    parse; here that raises ErrInvalidPubkey."""
    pub, ok = (ctx or default_context()).pubkey_parse_batch([bytes(pubkey)])
    if not ok[0]:
        raise ErrInvalidPubkey("invalid public key")
    return bytes([2 | (int(pub[0, 64]) & 1)]) + bytes(pub[0, 1:33])


class ErrInvalidKey(ValueError):
    """invalid private key"""


def _padded_key(prv) -> bytes:
    """math.PaddedBigBytes(prv.D, 32) (crypto/signature_cgo.go:58): an int, or bytes of at most 32, as 32
    big-endian bytes.  What has no such form is no valid key."""
    if isinstance(prv, int):
        if prv < 0 or prv >> 256:
            raise ErrInvalidKey("invalid private key")
        return prv.to_bytes(32, "big")
    prv = bytes(prv)
    if len(prv) > 32:
        raise ErrInvalidKey("invalid private key")
    return prv.rjust(32, b"\0")


def SignBatch(hashes, keys, ctx=None):
    """Batch crypto.Sign: hashes (n,32) uint8, keys (n,32) uint8 big-endian secret keys.  Returns
    (sigs (n,65) [R || S || V], status (n,)): ST_INVALID_KEY and a zero row for a key of 0 or >= n."""
    return (ctx or default_context()).ecdsa_sign_batch(hashes, keys)


def Sign(hash: bytes, prv, ctx=None) -> bytes:
    """crypto/signature_cgo.go:54-61 -> secp256k1.Sign (secp256.go:70-99): the 65-byte [R || S || V]
    signature of `hash` (32 bytes) by the secret key `prv` (an int, or up to 32 big-endian bytes), V in
    {0, 1}, with RFC 6979's nonce: byte for byte the reference's."""
    hash = bytes(hash)
    if len(hash) != 32:
        raise ErrInvalidMsgLen("invalid message length, need 32 bytes")
    key = _padded_key(prv)
    sig, st = SignBatch(np.frombuffer(hash, np.uint8)[None], np.frombuffer(key, np.uint8)[None], ctx)
    if st[0] != _lib.ST_OK:
        raise ErrInvalidKey("invalid private key")
    return bytes(sig[0])


def PubkeyFromSeckey(prv, ctx=None) -> bytes:
    """The 65-byte public key 04 || X || Y of a secret key (secp256k1_ec_pubkey_create, what
    crypto.ToECDSA derives)."""
    key = _padded_key(prv)
    pub, _, st = (ctx or default_context()).pubkey_create_batch(np.frombuffer(key, np.uint8)[None])
    if st[0] != _lib.ST_OK:
        raise ErrInvalidKey("invalid private key")
    return bytes(pub[0])


# the generator (crypto/secp256k1/curve.go:293-294 theCurve.Gx, Gy)
S256_GX = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
S256_GY = 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8


def ScalarMultBatch(points, scalars, ctx=None):
    """Batch BitCurve.ScalarMult: points (n,64) uint8 X || Y, scalars (n,32) uint8 big-endian.  Returns
    (out (n,64) X || Y of k P, status (n,)): ST_INVALID_KEY and a zero row for a scalar of 0 or >= n (where
    the reference returns (nil, nil)), ST_INVALID_CURVE and a zero row for a point off the curve (where
    the reference computes on another curve: include/gsv.h)."""
    return (ctx or default_context()).secp256k1_scalar_mul_batch(points, scalars)


def ScalarMult(x: int, y: int, k: bytes, ctx=None):
    """crypto/secp256k1/curve.go:221-254 BitCurve.ScalarMult: (x, y) of k (x, y), k big-endian bytes,
    left-padded to 32; more than 32 bytes raise ValueError (the reference panics).  (None, None) where the
    reference returns (nil, nil), a scalar of 0 or >= n, and for a point off the curve (the reference's
    result there is an artefact).  Coordinates are non-negative 256-bit values (math.ReadBits would keep
    the low 256 bits of a larger one; here that is a ValueError)."""
    k = bytes(k)
    if len(k) > 32:
        raise ValueError("can't handle scalars > 256 bits")
    if x < 0 or y < 0 or x >> 256 or y >> 256:
        raise ValueError("coordinates are 256-bit values")
    pt = np.frombuffer(x.to_bytes(32, "big") + y.to_bytes(32, "big"), np.uint8)[None]
    out, st = ScalarMultBatch(pt, np.frombuffer(k.rjust(32, b"\0"), np.uint8)[None], ctx)
    if st[0] != _lib.ST_OK:
        return None, None
    return int.from_bytes(bytes(out[0, :32]), "big"), int.from_bytes(bytes(out[0, 32:]), "big")


def ScalarBaseMult(k: bytes, ctx=None):
    """crypto/secp256k1/curve.go:257-259: ScalarMult on the generator."""
    return ScalarMult(S256_GX, S256_GY, k, ctx)


def PubkeyToAddress(pub65: bytes) -> bytes:
    """crypto/crypto.go:194-197: Keccak256(pub[1:])[12:]."""
    return Keccak256(bytes(pub65)[1:])[12:]


def ValidateSignatureValues(v: int, r: int, s: int, homestead: bool) -> bool:
    """crypto/crypto.go:181-192 (host-side predicate; the kernels apply the same rule per lane)."""
    n = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
    if r < 1 or s < 1:
        return False
    if homestead and s > n // 2:
        return False
    return r < n and s < n and v in (0, 1)


class EcrecoverPrecompile:
    """PrecompiledContract{RequiredGas, Run} for address 0x01 (core/vm/contracts.go:70-101)."""

    ECRECOVER_GAS = 3000  # params.EcrecoverGas

    def RequiredGas(self, input: bytes) -> int:
        return self.ECRECOVER_GAS

    def Run(self, input: bytes, ctx=None):
        """32-byte left-padded signer address, or None where the reference returns (nil, nil)."""
        out, ok = self.RunBatch([bytes(input)], ctx)
        return bytes(out[0]) if ok[0] else None

    def RunBatch(self, inputs, ctx=None):
        return (ctx or default_context()).ecrecover_precompile_batch(list(inputs))
