"""Mirror of the reference's precompiled contracts (core/vm/contracts.go), batched on the GPU.

    BigModExp.Run(input)          core/vm/contracts.go:226-252 (address 0x05, EIP-198)
    BigModExp.RunBatch(inputs)    the batch form: one output per precompile input
    BigModExp.RequiredGas(input)  core/vm/contracts.go:167-224, restated here (no C entry for gas)
    Sha256Hash / Ripemd160Hash / DataCopy     contracts.go:104-147 (0x02, 0x03, 0x04): RequiredGas, Run, RunBatch
    PrecompiledContractsHomestead / PrecompiledContractsByzantium   contracts.go:42-60
    RunPrecompiledContract(p, input, gas)     contracts.go:62-69: charge RequiredGas, then Run
    RunPrecompiledContracts(contracts, addrs, inputs, gas)   the same over a mixed batch: one batched call
                                              per precompile

The other five classes live in gsv.bn256 (Bn256Add / Bn256ScalarMul / Bn256Pairing) and gsv.crypto
(EcrecoverPrecompile).  The one departure from the reference (include/gsv.h): each of modexp's baseLen,
expLen and modLen is capped at MAX_LEN bytes; Run raises ErrModexpTooLong for an input above it, RunBatch
reports it per item.
"""
from __future__ import annotations

from . import _lib, default_context
from .bn256 import (Bn256Add, Bn256Pairing, Bn256ScalarMul, ErrBadPairingInput, ErrMalformedPoint, FALSE32,
                    TRUE32)
from .crypto import EcrecoverPrecompile

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


class ErrOutOfGas(Exception):
    """out of gas (core/vm/errors.go:22)"""


class _PerWordGas:
    """RequiredGas of the three precompiles priced by the 32-byte word (contracts.go:111-113, :126-128, :142-144)"""

    PER_WORD_GAS = 0
    BASE_GAS = 0

    def RequiredGas(self, input: bytes) -> int:
        return (len(input) + 31) // 32 * self.PER_WORD_GAS + self.BASE_GAS


class Sha256Hash(_PerWordGas):
    """PrecompiledContract{RequiredGas, Run} for address 0x02 (core/vm/contracts.go:104-117)."""

    PER_WORD_GAS = 12  # params.Sha256PerWordGas (params/protocol_params.go:70)
    BASE_GAS = 60      # params.Sha256BaseGas (:69)

    def RunBatch(self, inputs, ctx=None):
        """(n, 32) uint8: one sha256_batch call"""
        return (ctx or default_context()).sha256_batch([bytes(x) for x in inputs])

    def Run(self, input: bytes, ctx=None) -> bytes:
        return bytes(self.RunBatch([input], ctx)[0])


class Ripemd160Hash(_PerWordGas):
    """PrecompiledContract{RequiredGas, Run} for address 0x03 (core/vm/contracts.go:119-133): the digest
    left-padded to 32 bytes."""

    PER_WORD_GAS = 120  # params.Ripemd160PerWordGas (params/protocol_params.go:72)
    BASE_GAS = 600      # params.Ripemd160BaseGas (:71)

    def RunBatch(self, inputs, ctx=None):
        """(n, 32) uint8 rows of 12 zero bytes and the digest: one ripemd160_batch call"""
        return (ctx or default_context()).ripemd160_batch([bytes(x) for x in inputs])

    def Run(self, input: bytes, ctx=None) -> bytes:
        return bytes(self.RunBatch([input], ctx)[0])


class DataCopy(_PerWordGas):
    """PrecompiledContract{RequiredGas, Run} for address 0x04 (core/vm/contracts.go:135-147): the identity,
    which touches no device."""

    PER_WORD_GAS = 3  # params.IdentityPerWordGas (params/protocol_params.go:74)
    BASE_GAS = 15     # params.IdentityBaseGas (:73)

    def RunBatch(self, inputs, ctx=None):
        return [bytes(x) for x in inputs]

    def Run(self, input: bytes, ctx=None) -> bytes:
        return bytes(input)


def _address(n: int) -> bytes:
    """common.BytesToAddress([]byte{n})"""
    return bytes(19) + bytes([n])


# core/vm/contracts.go:42-47 and :51-60
PrecompiledContractsHomestead = {_address(1): EcrecoverPrecompile(), _address(2): Sha256Hash(),
                                 _address(3): Ripemd160Hash(), _address(4): DataCopy()}
PrecompiledContractsByzantium = {**PrecompiledContractsHomestead, _address(5): BigModExp(), _address(6): Bn256Add(),
                                 _address(7): Bn256ScalarMul(), _address(8): Bn256Pairing()}


def _run_family(p, inputs, ctx):
    """[(ret, err)] of p.Run over `inputs`, what the reference's Run returns for each, from ONE batched call
    of p's family (none where no input reaches the device)"""
    if isinstance(p, EcrecoverPrecompile):  # (nil, nil) where recovery fails (contracts.go:90-98)
        out, ok = p.RunBatch(inputs, ctx)
        return [(bytes(out[i]) if ok[i] else b"", None) for i in range(len(inputs))]
    if isinstance(p, BigModExp):
        out, st = p.RunBatch(inputs, ctx)
        return [(None, ErrModexpTooLong(_lib.STATUS_STRINGS[_lib.ST_MODEXP_TOO_LONG]))
                if st[i] == _lib.ST_MODEXP_TOO_LONG else (out[i], None) for i in range(len(inputs))]
    if isinstance(p, (Bn256Add, Bn256ScalarMul)):
        out, st = p.RunBatch(inputs, ctx)
        return [(out[i].tobytes(), None) if st[i] == _lib.ST_OK else (None, ErrMalformedPoint("bn256: malformed point"))
                for i in range(len(inputs))]
    if isinstance(p, Bn256Pairing):  # the size rule precedes every point (contracts.go:335-337)
        res = [(None, ErrBadPairingInput("bad elliptic curve pairing size")) if len(x) % 192 else None for x in inputs]
        idx = [i for i, r in enumerate(res) if r is None]
        if idx:
            v = p.RunBatch([inputs[i] for i in idx], ctx)
            for k, i in enumerate(idx):
                res[i] = (None, ErrMalformedPoint("bn256: malformed point")) if v[k] == _lib.PAIRING_BAD_INPUT else \
                    (TRUE32 if v[k] == _lib.PAIRING_TRUE else FALSE32, None)
        return res
    # Sha256Hash, Ripemd160Hash, DataCopy, and any contract with a RunBatch of one output per input
    out = p.RunBatch(inputs, ctx)
    return [(bytes(out[i]), None) for i in range(len(inputs))]


def RunPrecompiledContracts(contracts, addrs, inputs, gas, ctx=None):
    """RunPrecompiledContract (core/vm/contracts.go:62-69) over a mixed batch: item i calls the contract at
    the 20-byte address addrs[i] of `contracts` (PrecompiledContractsByzantium, ...) with inputs[i] and
    gas[i].  Returns [(ret, err, gas_left)] in input order.  An item whose RequiredGas is above its gas is
    (None, ErrOutOfGas, its gas unchanged) and never reaches the device; the others are grouped by address
    and each group runs as one batched call.  ret and err are what the reference's Run returns: bytes and
    None, or None and the error (an instance of the class that the contract's own Run raises); ecrecover's
    (nil, nil) is (b"", None).  An address that `contracts` does not hold raises KeyError before any work."""
    addrs = [bytes(a) for a in addrs]
    inputs = [bytes(x) for x in inputs]
    gas = [int(g) for g in gas]
    if not len(addrs) == len(inputs) == len(gas):
        raise ValueError("addrs, inputs and gas batch sizes differ")
    ps = [contracts[a] for a in addrs]  # KeyError here, before any work
    res = [None] * len(addrs)
    groups = {}
    for i, p in enumerate(ps):
        need = p.RequiredGas(inputs[i])
        if need > gas[i]:  # Contract.UseGas fails and leaves the gas as it was (core/vm/contract.go)
            res[i] = (None, ErrOutOfGas("out of gas"), gas[i])
        else:
            gas[i] -= need
            groups.setdefault(addrs[i], []).append(i)
    for a, idx in groups.items():
        for i, (ret, err) in zip(idx, _run_family(contracts[a], [inputs[i] for i in idx], ctx)):
            res[i] = (ret, err, gas[i])
    return res


def RunPrecompiledContract(p, input: bytes, gas: int, ctx=None):
    """(ret, err, gas_left) of one call of the contract p (core/vm/contracts.go:62-69)"""
    return RunPrecompiledContracts({_address(0): p}, [_address(0)], [input], [gas], ctx)[0]
