"""Mirror of the reference's BN254 pairing entry points, batched on the GPU.

    PairingCheck(a, b)          crypto/bn256/bn256_fast.go -> cloudflare/bn256.go:313-327
    PairingCheckBatch(inputs)   the batch form: one verdict per precompile input
    Bn256Pairing.Run(input)     core/vm/contracts.go:333-360 (true32Byte / false32Byte / error)

    G1Add(a, b) / G1ScalarMult(a, k)   cloudflare/bn256.go:62-78 over 64-byte encodings
    Bn256Add.Run / Bn256ScalarMul.Run  core/vm/contracts.go:274-312 (64 bytes / error)

Points use the precompile encoding: G1 = x || y, G2 = x.imag || x.real || y.imag || y.real,
32-byte big-endian words (bn256.go:120-164, :256-306).  Malformed points raise
ErrMalformedPoint where the reference's Unmarshal returns an error.
"""
from __future__ import annotations

import numpy as np

from . import _lib, default_context


class ErrBadPairingInput(ValueError):
    """bad elliptic curve pairing size (core/vm/contracts.go:315, errBadPairingInput)"""


class ErrMalformedPoint(ValueError):
    """bn256: coordinate exceeds modulus / malformed point (cloudflare/bn256.go)"""


TRUE32 = bytes(31) + b"\x01"
FALSE32 = bytes(32)


def PairingCheckBatch(inputs, ctx=None) -> np.ndarray:
    return (ctx or default_context()).pairing_check_batch(list(inputs))


def PairingCheck(a, b, ctx=None) -> bool:
    """a: list of 64-byte G1 encodings, b: list of 128-byte G2 encodings."""
    if len(a) != len(b):
        raise ValueError("PairingCheck: len(a) != len(b)")
    inp = b"".join(bytes(x) + bytes(y) for x, y in zip(a, b))
    v = PairingCheckBatch([inp], ctx)[0]
    if v == _lib.PAIRING_BAD_INPUT:
        raise ErrMalformedPoint("bn256: malformed point")
    return bool(v == _lib.PAIRING_TRUE)


class Bn256Pairing:
    """PrecompiledContract{RequiredGas, Run} for address 0x08 (core/vm/contracts.go:325-360)."""

    PAIRING_BASE_GAS = 100000   # params.Bn256PairingBaseGas
    PAIRING_PER_POINT_GAS = 80000  # params.Bn256PairingPerPointGas

    def RequiredGas(self, input: bytes) -> int:
        return self.PAIRING_BASE_GAS + (len(input) // 192) * self.PAIRING_PER_POINT_GAS

    def Run(self, input: bytes, ctx=None) -> bytes:
        if len(input) % 192:
            raise ErrBadPairingInput("bad elliptic curve pairing size")
        v = PairingCheckBatch([bytes(input)], ctx)[0]
        if v == _lib.PAIRING_BAD_INPUT:  # newCurvePoint / newTwistPoint error (contracts.go:344-351)
            raise ErrMalformedPoint("bn256: malformed point")
        return TRUE32 if v == _lib.PAIRING_TRUE else FALSE32

    def RunBatch(self, inputs, ctx=None) -> np.ndarray:
        """(n,) uint8 verdicts PAIRING_FALSE / PAIRING_TRUE / PAIRING_BAD_INPUT of inputs whose lengths are
        multiples of 192 (Run refuses the others before the device): one pairing_check_batch call"""
        return PairingCheckBatch([bytes(x) for x in inputs], ctx)


def G1Add(a: bytes, b: bytes, ctx=None) -> bytes:
    """Marshal(Unmarshal(a) + Unmarshal(b)) over 64-byte G1 encodings (bn256.go:62-67)."""
    return Bn256Add().Run(bytes(a).ljust(64, b"\0")[:64] + bytes(b), ctx)


def G1ScalarMult(a: bytes, k: int, ctx=None) -> bytes:
    """Marshal(k * Unmarshal(a)) (bn256.go:70-78); k is taken mod 2^256 as the precompile's word."""
    return Bn256ScalarMul().Run(bytes(a).ljust(64, b"\0")[:64] + (int(k) % 2**256).to_bytes(32, "big"), ctx)


class Bn256Add:
    """PrecompiledContract{RequiredGas, Run} for address 0x06 (core/vm/contracts.go:266-289)."""

    GAS = 500  # params.Bn256AddGas (params/protocol_params.go:76)

    def RequiredGas(self, input: bytes) -> int:
        return self.GAS

    def Run(self, input: bytes, ctx=None) -> bytes:
        out, st = (ctx or default_context()).bn256_add_batch([bytes(input)])
        if st[0] != _lib.ST_OK:  # newCurvePoint error (contracts.go:276-283)
            raise ErrMalformedPoint("bn256: malformed point")
        return out[0].tobytes()

    def RunBatch(self, inputs, ctx=None):
        """(out (n,64) uint8, status (n,)): ST_BN_BAD_INPUT and a zero row where Run raises; one
        bn256_add_batch call"""
        return (ctx or default_context()).bn256_add_batch([bytes(x) for x in inputs])


class Bn256ScalarMul:
    """PrecompiledContract{RequiredGas, Run} for address 0x07 (core/vm/contracts.go:291-312)."""

    GAS = 40000  # params.Bn256ScalarMulGas (params/protocol_params.go:77)

    def RequiredGas(self, input: bytes) -> int:
        return self.GAS

    def Run(self, input: bytes, ctx=None) -> bytes:
        out, st = (ctx or default_context()).bn256_scalar_mul_batch([bytes(input)])
        if st[0] != _lib.ST_OK:  # newCurvePoint error (contracts.go:299-303)
            raise ErrMalformedPoint("bn256: malformed point")
        return out[0].tobytes()

    def RunBatch(self, inputs, ctx=None):
        """(out (n,64) uint8, status (n,)) as Bn256Add.RunBatch; one bn256_scalar_mul_batch call"""
        return (ctx or default_context()).bn256_scalar_mul_batch([bytes(x) for x in inputs])
