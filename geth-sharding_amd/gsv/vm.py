"""Mirror of the reference's bigModExp precompile (address 0x05, EIP-198), batched on the GPU.

    BigModExp.Run(input)          core/vm/contracts.go:226-252
    BigModExp.RunBatch(inputs)    the batch form: one output per precompile input
    BigModExp.RequiredGas(input)  core/vm/contracts.go:167-224, restated here (no C entry for gas)

It sits beside gsv.bn256.Bn256Add / Bn256ScalarMul / Bn256Pairing and gsv.crypto.EcrecoverPrecompile.  The
one departure from the reference (include/gsv.h): each of baseLen, expLen and modLen is capped at
MAX_LEN bytes; Run raises ErrModexpTooLong for an input above it, RunBatch reports it per item.
"""
from __future__ import annotations

from . import _lib, default_context

MAX_LEN = _lib.MODEXP_MAX_LEN


class ErrModexpTooLong(ValueError):
    """a modexp length above GSV_MODEXP_MAX_LEN (GSV_ST_MODEXP_TOO_LONG): run this item elsewhere"""


def _get_data(data: bytes, start: int, size: int) -> bytes:
    """getData (core/vm/common.go:37-47)"""
    start = min(start, len(data))
    end = min(start + size, len(data))
    return data[start:end].ljust(size, b"\0")


class BigModExp:
    """PrecompiledContract{RequiredGas, Run} for address 0x05 (core/vm/contracts.go:149-252)."""

    QUAD_COEFF_DIV = 20  # params.ModExpQuadCoeffDiv (params/protocol_params.go:75)

    def RequiredGas(self, input: bytes) -> int:
        input = bytes(input)
        base_len, exp_len, mod_len = (int.from_bytes(_get_data(input, at, 32), "big") for at in (0, 32, 64))
        body = input[96:] if len(input) > 96 else b""
        # the head 32 bytes of exp, for the adjusted exponent length (:178-199); getData takes Uint64()s
        u64 = (1 << 64) - 1
        if len(body) <= base_len:
            head = 0
        elif exp_len > 32:
            head = int.from_bytes(_get_data(body, base_len & u64, 32), "big")
        else:
            head = int.from_bytes(_get_data(body, base_len & u64, exp_len & u64), "big")
        msb = head.bit_length() - 1 if head else 0
        adj = (8 * (exp_len - 32) if exp_len > 32 else 0) + msb
        gas = max(mod_len, base_len)
        if gas <= 64:
            gas = gas * gas
        elif gas <= 1024:
            gas = gas * gas // 4 + (96 * gas - 3072)
        else:
            gas = gas * gas // 16 + (480 * gas - 199680)
        gas = gas * max(adj, 1) // self.QUAD_COEFF_DIV
        return u64 if gas.bit_length() > 64 else gas

    def RunBatch(self, inputs, ctx=None):
        """(outputs: list of bytes, status (n,) uint8: ST_OK or ST_MODEXP_TOO_LONG with an empty output)"""
        return (ctx or default_context()).modexp_batch(list(inputs))

    def Run(self, input: bytes, ctx=None) -> bytes:
        out, st = self.RunBatch([bytes(input)], ctx)
        if st[0] == _lib.ST_MODEXP_TOO_LONG:
            raise ErrModexpTooLong(_lib.STATUS_STRINGS[_lib.ST_MODEXP_TOO_LONG])
        return out[0]
