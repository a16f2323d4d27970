"""The seeded corpus of modexp precompile inputs shared by tests/test_modexp_cpu.py and
tests/test_gpu_modexp.py: both sides of every width-class edge and limb edge of the modulus, bases shorter,
equal and longer than it, odd / even / power-of-two / degenerate moduli, and the encodings getData pads or
cuts.  Expectations are never stored here: they come from tests/modexp_model.py."""
import random

MOD_LENS = (1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024)
EXP_LENS = (0, 1, 3, 32, 33, 64)
MOD_KINDS = ("odd", "top0", "ff", "one", "zero", "k1", "k31", "k32", "k33", "kmax", "pow2", "2q")
BASE_KINDS = ("zero", "one", "m-1", "m", "m+1", "longer", "ff")
EXP_KINDS = ("zero", "one", "two", "three", "f4", "lead0", "ff")
SMALL_EXP_FROM = 257  # moduli this long or longer (the 512- and 1024-byte classes) get exponents <= 16 bits


def base_lens(mod_len):
    return sorted({min(v, 1024) for v in (0, 1, mod_len - 1, mod_len, mod_len + 1, 2 * mod_len + 3, 1024)})


def word(n):
    return int(n).to_bytes(32, "big")


def encode(base: bytes, exp: bytes, mod: bytes) -> bytes:
    return word(len(base)) + word(len(exp)) + word(len(mod)) + base + exp + mod


def modulus(rng, kind, n):
    """n bytes"""
    bits = 8 * n
    top = 1 << (bits - 1)
    if kind == "odd":
        v = rng.getrandbits(bits) | top | 1
    elif kind == "top0":
        v = (rng.getrandbits(bits) >> 8) | 1
    elif kind == "ff":
        v = (1 << bits) - 1
    elif kind == "one":
        v = 1
    elif kind == "zero":
        v = 0
    elif kind in ("k1", "k31", "k32", "k33"):
        k = min(int(kind[1:]), bits - 1)
        v = ((rng.getrandbits(bits) | top) >> k | 1) << k
    elif kind == "kmax":
        v = top  # k = 8 n - 1
    elif kind == "pow2":
        v = 1 << rng.randrange(bits)
    else:  # 2q
        v = ((rng.getrandbits(bits - 1) | (top >> 1) | 1) << 1) if bits > 1 else 0
    return (v % (1 << bits)).to_bytes(n, "big")


def base(rng, kind, n, m):
    """n bytes; where m - 1, m, m + 1 do not fit they are cut to the low n bytes"""
    if kind == "zero":
        v = 0
    elif kind == "one":
        v = 1
    elif kind in ("m-1", "m", "m+1"):
        v = m + {"m-1": -1, "m": 0, "m+1": 1}[kind]
    elif kind == "longer":
        v = rng.getrandbits(8 * n) | (1 << (8 * n - 1)) if n else 0
    else:
        v = (1 << (8 * n)) - 1
    return (v % (1 << (8 * n))).to_bytes(n, "big") if n else b""


def exponent(rng, kind, n, small):
    """n bytes; `small` keeps the value to 16 bits"""
    cap = min(8 * n, 16) if small else 8 * n
    if kind == "zero" or n == 0:
        v = 0
    elif kind in ("one", "two", "three"):
        v = {"one": 1, "two": 2, "three": 3}[kind]
    elif kind == "f4":
        v = 65537 if n >= 3 else 3
    elif kind == "lead0":
        v = rng.getrandbits(max(cap // 2, 1))
    else:
        v = (1 << cap) - 1
    return (v % (1 << (8 * n))).to_bytes(n, "big") if n else b""


def _item(rng, ml, bl, el, mk, bk, ek):
    m = modulus(rng, mk, ml)
    b = base(rng, bk, bl, int.from_bytes(m, "big"))
    e = exponent(rng, ek, el, ml >= SMALL_EXP_FROM)
    return ("ml=%d bl=%d el=%d %s/%s/%s" % (ml, bl, el, mk, bk, ek), encode(b, e, m))


def encodings(rng):
    """what getData pads, cuts or ignores"""
    m = modulus(rng, "odd", 32)
    b = base(rng, "longer", 33, 0)
    e = exponent(rng, "ff", 3, False)
    full = encode(b, e, m)
    out = [("empty", b""), ("1 byte", b"\x01"), ("95 bytes", full[:95]), ("96 bytes", full[:96]),
           ("97 bytes", full[:97]), ("cut in base", full[:96 + 20]), ("cut in exp", full[:96 + 33 + 1]),
           ("cut in mod", full[:96 + 33 + 3 + 7]), ("cut in mod, one byte left", full[:96 + 33 + 3 + 1]),
           ("mod missing", full[:96 + 33 + 3]), ("body longer", full + bytes(range(1, 40)))]
    junk = bytes(range(1, 25))  # the first 24 bytes of a length word are ignored
    out.append(("junk in length words", junk + full[24:32] + junk + full[56:64] + junk + full[88:96] + full[96:]))
    for at in (0, 32, 64):
        for v in (1025, 2 ** 63, 2 ** 64 - 1):
            hdr = bytearray(full[:96])
            hdr[at:at + 32] = word(v)
            out.append(("length word %d = %d" % (at // 32, v), bytes(hdr) + full[96:]))
    # a length of 2^64 is 0 after Uint64()
    hdr = bytearray(full[:96])
    hdr[0:32] = word(2 ** 64)
    out.append(("base length 2^64 reads as 0", bytes(hdr) + full[96:]))
    out.append(("all lengths 0 with a body", word(0) * 3 + b"\x05\x06"))
    out.append(("base 0 mod 0 exp 5", word(0) + word(5) + word(0) + b"\x01" * 5))
    out.append(("mod 0 base 2", word(2) + word(1) + word(0) + b"\x01\x02\x03"))
    out.append(("the cap itself", encode(bytes([7]) * 1024, b"\x03", modulus(rng, "odd", 1024))))
    return out


def items(seed=198):
    rng = random.Random(seed)
    out = []
    for ml in MOD_LENS:
        for bl in base_lens(ml):
            for el in EXP_LENS:
                for _ in range(2):
                    out.append(_item(rng, ml, bl, el, rng.choice(MOD_KINDS), rng.choice(BASE_KINDS),
                                     rng.choice(EXP_KINDS)))
        bls = base_lens(ml)
        for mk in MOD_KINDS:
            out.append(_item(rng, ml, rng.choice(bls), rng.choice(EXP_LENS), mk, rng.choice(BASE_KINDS),
                             rng.choice(EXP_KINDS)))
        for bk in BASE_KINDS:
            out.append(_item(rng, ml, rng.choice(bls), rng.choice(EXP_LENS), rng.choice(MOD_KINDS), bk,
                             rng.choice(EXP_KINDS)))
        for ek in EXP_KINDS:
            out.append(_item(rng, ml, rng.choice(bls), rng.choice(EXP_LENS[1:]), rng.choice(MOD_KINDS),
                             rng.choice(BASE_KINDS), ek))
    out += encodings(rng)
    return out


def mixed_wave(seed=5, n=193, ml=32):
    """n items of one width class whose lanes take every path: odd, even and power-of-two moduli and
    m in {0, 1} in turn, exponent bit lengths running from 0 to 256"""
    rng = random.Random(seed)
    kinds = ("odd", "k1", "pow2", "zero", "2q", "one", "k33", "kmax")
    out = []
    for i in range(n):
        m = modulus(rng, kinds[i % len(kinds)], ml)
        bits = (i * 256) // (n - 1)
        e = (rng.getrandbits(bits) | (1 << (bits - 1))) if bits else 0
        b = rng.getrandbits(8 * ml)
        out.append(encode(b.to_bytes(ml, "big"), e.to_bytes(32, "big"), m))
    return out
