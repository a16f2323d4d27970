"""bigModExp (core/vm/contracts.go:149-252) restated with Python integers: Run, RequiredGas, and the one
departure of the library (include/gsv.h): an item with a length above MAX_LEN gets ST_TOO_LONG and an
empty output."""
ST_OK = 0
ST_TOO_LONG = 15
MAX_LEN = 1024
QUAD_COEFF_DIV = 20  # params.ModExpQuadCoeffDiv (params/protocol_params.go)
MAX_U64 = 2 ** 64 - 1


def get_data(data: bytes, start: int, size: int) -> bytes:
    """getData (core/vm/common.go:37-47): data[start : start + size], right-padded with zeros to size"""
    start = min(start, len(data))
    end = min(start + size, len(data))
    return data[start:end].ljust(size, b"\0")


def lengths(inp: bytes):
    """new(big.Int).SetBytes(getData(input, at, 32)).Uint64(): the low 64 bits of each length word"""
    return tuple(int.from_bytes(get_data(inp, at, 32), "big") & MAX_U64 for at in (0, 32, 64))


def operands(inp: bytes):
    base_len, exp_len, mod_len = lengths(inp)
    body = inp[96:] if len(inp) > 96 else b""
    return (int.from_bytes(get_data(body, 0, base_len), "big"),
            int.from_bytes(get_data(body, base_len, exp_len), "big"),
            int.from_bytes(get_data(body, base_len + exp_len, mod_len), "big"))


def run(inp: bytes) -> bytes:
    """bigModExp.Run (contracts.go:226-252), for lengths a Python integer can hold"""
    inp = bytes(inp)
    base_len, exp_len, mod_len = lengths(inp)
    if base_len == 0 and mod_len == 0:
        return b""
    base, exp, mod = operands(inp)
    if mod == 0:
        return bytes(mod_len)
    return pow(base, exp, mod).to_bytes(mod_len, "big")


def status(inp: bytes) -> int:
    return ST_TOO_LONG if max(lengths(bytes(inp))) > MAX_LEN else ST_OK


def run_capped(inp: bytes):
    """(status, output) as the library gives them"""
    st = status(inp)
    return st, (b"" if st else run(inp))


def required_gas(inp: bytes) -> int:
    """bigModExp.RequiredGas (contracts.go:167-224); the lengths are whole 256-bit words here"""
    inp = bytes(inp)
    base_len, exp_len, mod_len = (int.from_bytes(get_data(inp, at, 32), "big") for at in (0, 32, 64))
    body = inp[96:] if len(inp) > 96 else b""
    if len(body) <= base_len:
        exp_head = 0
    elif exp_len > 32:
        exp_head = int.from_bytes(get_data(body, base_len & MAX_U64, 32), "big")
    else:
        exp_head = int.from_bytes(get_data(body, base_len & MAX_U64, exp_len & MAX_U64), "big")
    msb = exp_head.bit_length() - 1 if exp_head else 0
    adj = 8 * (exp_len - 32) if exp_len > 32 else 0
    adj += msb
    g = max(mod_len, base_len)
    if g <= 64:
        g = g * g
    elif g <= 1024:
        g = g * g // 4 + (96 * g - 3072)
    else:
        g = g * g // 16 + (480 * g - 199680)
    g = g * max(adj, 1) // QUAD_COEFF_DIV
    return MAX_U64 if g.bit_length() > 64 else g
