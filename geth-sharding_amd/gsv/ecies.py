"""Mirror of the reference's ECIES (crypto/ecies), batched on the GPU.

    GenerateShared(prv, pub, skLen, macLen)   crypto/ecies/ecies.go:121-138: the ECDH shared secret
    GenerateSharedBatch(prvs, pubs)           batch form: per-item status codes
    DeriveKeysBatch(prvs, pubs)               the key derivation of ecies.Encrypt / Decrypt
                                              (ecies.go:264-277, 347-356) for ECIES_AES128_SHA256
                                              (params.go:69-76) with s1 empty: Ke (16 bytes), Km (32 bytes)
    Decrypt(prv, c, s1, s2)                   ecies.go:295-366: PrivateKey.Decrypt, AES-128-CTR and the
    Encrypt(rand, pub, m, s1, s2)             HMAC-SHA256 tag included; ecies.go:251-292
    DecryptBatch(prvs, cts, s2s)              batch forms: per-item status codes (include/gsv.h numbers
    EncryptBatch(msgs, pubs, ephs, ivs, s2s)  Decrypt's checks); the ephemeral keys and IVs are the caller's

The multiplication is the reference's secp256k1_ext_scalar_mul (crypto/secp256k1/ext.h:104-142) behind
BitCurve.ScalarMult.  One divergence: a public point that is not on the curve is refused
(ErrInvalidCurve, ST_INVALID_CURVE), where the reference multiplies on another curve; its callers check
IsOnCurve first (ecies.go:337), and Encrypt refuses it too.  A non-empty s1 raises NotImplementedError.
Encrypt draws a 32-byte key from `rand` until it is in [1, n), then a 16-byte IV: the reference's
distribution, but not its way of consuming rand's stream (GenerateKey reads 40 bytes and reduces them).
"""
from __future__ import annotations

import numpy as np

from . import _lib, default_context
from .crypto import _padded_key


class ErrInvalidCurve(ValueError):
    """ecies: invalid elliptic curve"""


class ErrInvalidMessage(ValueError):
    """ecies: invalid message"""


class ErrInvalidPublicKey(ValueError):
    """ecies: invalid public key"""


class ErrSharedKeyTooBig(ValueError):
    """ecies: shared key params are too big"""


class ErrSharedKeyIsPointAtInfinity(ValueError):
    """ecies: shared key is point at infinity"""


MAX_SHARED_KEY_LENGTH = 32  # MaxSharedKeyLength (ecies.go:116-118): (BitSize + 7) / 8


def _pub64(pub) -> bytes:
    """A public point as 64 bytes X || Y: 64 bytes, 65 bytes 04 || X || Y, or a pair of ints."""
    if isinstance(pub, tuple):
        x, y = pub
        if x < 0 or y < 0 or x >> 256 or y >> 256:
            raise ErrInvalidCurve("ecies: invalid elliptic curve")
        return x.to_bytes(32, "big") + y.to_bytes(32, "big")
    pub = bytes(pub)
    if len(pub) == 65 and pub[0] == 4:
        pub = pub[1:]
    if len(pub) != 64:
        raise ValueError("a public point is 64 bytes X || Y, 04 || X || Y, or a pair (x, y)")
    return pub


def GenerateSharedBatch(prvs, pubs, ctx=None):
    """Batch ECDH: prvs (n,32) uint8 big-endian secret keys, pubs (n,64) uint8 X || Y.  Returns
    (shared (n,32) X left-padded with zeros, status (n,)): ST_INVALID_KEY (the reference's
    ErrSharedKeyIsPointAtInfinity: a key of 0 or >= n) or ST_INVALID_CURVE, and a zero row for both."""
    shared, _, st = (ctx or default_context()).ecdh_batch(pubs, prvs, want_shared=True, want_keys=False)
    return shared, st


def DeriveKeysBatch(prvs, pubs, ctx=None):
    """The keys ecies.Encrypt(rand, pub, m, nil, nil) / Decrypt and the RLPx handshake derive from the
    shared secret: K = concatKDF(SHA256, X, nil, 32), Ke = K[:16], Km = SHA256(K[16:]).  Returns
    (Ke (n,16), Km (n,32), status (n,)); zero rows where the status is not ST_OK."""
    _, k48, st = (ctx or default_context()).ecdh_batch(pubs, prvs, want_shared=False, want_keys=True)
    return np.ascontiguousarray(k48[:, :16]), np.ascontiguousarray(k48[:, 16:]), st


def GenerateShared(prv, pub, skLen: int, macLen: int, ctx=None) -> bytes:
    """crypto/ecies/ecies.go:121-138: the ECDH shared secret of the secret key `prv` (an int, or up to 32
    big-endian bytes) and the public point `pub` (64 bytes X || Y, 65 bytes 04 || X || Y, or (x, y)), as
    skLen + macLen bytes: X's bytes right-aligned in a zero buffer (ecies.go:134-137).

    skLen + macLen > 32 raises ErrSharedKeyTooBig.  The reference's copy(sk[len(sk)-len(skBytes):], ...)
    panics when X has more bytes than skLen + macLen, so only the sum that cannot is accepted: 32 (any other
    raises ValueError).  The reference's callers all pass 16 + 16, or 32 + 32, which is too big."""
    if skLen < 0 or macLen < 0:
        raise ValueError("negative key length")
    if skLen + macLen > MAX_SHARED_KEY_LENGTH:
        raise ErrSharedKeyTooBig("ecies: shared key params are too big")
    if skLen + macLen != MAX_SHARED_KEY_LENGTH:
        raise ValueError("skLen + macLen below 32: the reference panics whenever X is longer than that")
    key = _padded_key(prv)
    shared, st = GenerateSharedBatch(np.frombuffer(key, np.uint8)[None], np.frombuffer(_pub64(pub), np.uint8)[None],
                                     ctx)
    if st[0] == _lib.ST_INVALID_KEY:
        raise ErrSharedKeyIsPointAtInfinity("ecies: shared key is point at infinity")
    if st[0] != _lib.ST_OK:
        raise ErrInvalidCurve("ecies: invalid elliptic curve")
    # x.Bytes() right-aligned in skLen + macLen = 32 zero bytes: the 32-byte big-endian X itself
    return bytes(shared[0])


def _raise_status(st: int):
    if st == _lib.ST_INVALID_MESSAGE:
        raise ErrInvalidMessage("ecies: invalid message")
    if st == _lib.ST_INVALID_PUBKEY:
        raise ErrInvalidPublicKey("ecies: invalid public key")
    if st == _lib.ST_INVALID_CURVE:
        raise ErrInvalidCurve("ecies: invalid elliptic curve")
    if st == _lib.ST_INVALID_KEY:
        raise ErrSharedKeyIsPointAtInfinity("ecies: shared key is point at infinity")
    raise ValueError(_lib.STATUS_STRINGS.get(st, f"status {st}"))


def _no_s1(s1):
    if s1:
        raise NotImplementedError("a non-empty s1 (the KDF's shared information) is not built")


def DecryptBatch(prvs, cts, s2s=None, ctx=None):
    """Batch Decrypt: prvs (n,32) uint8 big-endian secret keys, cts a list of ciphertexts, s2s a list of byte
    strings or None (every s2 empty).  Returns (msgs, status (n,)); msgs[i] is b"" where the status is not
    ST_OK: ST_INVALID_MESSAGE, ST_INVALID_PUBKEY, ST_INVALID_CURVE or ST_INVALID_KEY."""
    return (ctx or default_context()).ecies_decrypt_batch(cts, prvs, s2s)


def EncryptBatch(msgs, pubs, ephs, ivs, s2s=None, ctx=None):
    """Batch Encrypt with the caller's randomness: msgs a list of messages, pubs (n,64) uint8 recipient points
    X || Y, ephs (n,32) ephemeral secret keys, ivs (n,16).  Returns (cts, status (n,)); a failed item's
    ciphertext is 113 + len(m) zero bytes: ST_INVALID_KEY (ephemeral key 0 or >= n), ST_INVALID_CURVE,
    ST_INVALID_MESSAGE (an empty message)."""
    return (ctx or default_context()).ecies_encrypt_batch(msgs, pubs, ephs, ivs, s2s)


def Decrypt(prv, c, s1=None, s2=None, ctx=None) -> bytes:
    """crypto/ecies/ecies.go:295-366 PrivateKey.Decrypt: `prv` an int or up to 32 big-endian bytes.  Raises
    ErrInvalidMessage, ErrInvalidPublicKey, ErrInvalidCurve or ErrSharedKeyIsPointAtInfinity (a key of 0 or
    >= n).  A non-empty s1 raises NotImplementedError."""
    _no_s1(s1)
    key = np.frombuffer(_padded_key(prv), np.uint8)[None]
    msgs, st = DecryptBatch(key, [bytes(c)], [bytes(s2 or b"")], ctx)
    if st[0] != _lib.ST_OK:
        _raise_status(int(st[0]))
    return msgs[0]


_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


def Encrypt(rand, pub, m, s1=None, s2=None, ctx=None) -> bytes:
    """crypto/ecies/ecies.go:251-292 Encrypt: `rand` a callable n -> n random bytes (os.urandom), `pub` as for
    GenerateShared.  An empty message returns b"", as the reference returns nil (ecies.go:280).  A non-empty
    s1 raises NotImplementedError."""
    _no_s1(s1)
    pub = np.frombuffer(_pub64(pub), np.uint8)[None]
    while True:
        eph = bytes(rand(32))
        if len(eph) != 32:
            raise ValueError("rand(32) did not return 32 bytes")
        if 0 < int.from_bytes(eph, "big") < _N:
            break
    iv = bytes(rand(16))
    if len(iv) != 16:
        raise ValueError("rand(16) did not return 16 bytes")
    cts, st = EncryptBatch([bytes(m)], pub, np.frombuffer(eph, np.uint8)[None], np.frombuffer(iv, np.uint8)[None],
                           [bytes(s2 or b"")], ctx)
    if st[0] == _lib.ST_INVALID_MESSAGE:
        return b""
    if st[0] != _lib.ST_OK:
        _raise_status(int(st[0]))
    return cts[0]
