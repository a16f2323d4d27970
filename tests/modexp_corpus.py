"""The seeded corpus of modexp precompile inputs shared by tests/test_modexp_cpu.py and
tests/test_gpu_modexp.py: both sides of every width-class edge and limb edge of the modulus, bases shorter,
equal and longer than it, odd / even / power-of-two / degenerate moduli, and the encodings getData pads or
cuts; and the shapes of the device form (dev_shapes, rows, two_trip_rows), which tests/test_gpu_modexp_shapes.py
launches and tests/test_modexp_cpu.py feeds to the host build of the arithmetic: modulus lengths at every
residue mod 4 on both sides of every class, bases with a partial top piece, and a launch whose first waves
come round a second time.  Expectations are never stored here: they come from tests/modexp_model.py."""
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


# ---------------------------------------------------------------- shapes of the device form
# A launch of the device form has one (bl, el, ml) for all its rows, so these lengths reach the kernel as they
# are: nothing pads them to a class width as the host form's grouping does.
NCLASS = 6
WIDE_EXP_FIELD = 1024  # an exponent field this wide holds a value of at most 16 bits behind its zero bytes
# Classes whose modulus lengths are thinned to one length = 1 (mod 4) just above the class's lower edge and
# one = 3 (mod 4) just below its upper edge.  Empty: every class runs its eight lengths (the durations are in
# the commit that added tests/test_gpu_modexp_shapes.py).
THIN_CLASSES = ()
BASE_LEN_KINDS = ("0", "1", "ml-1", "ml+1", "4L+1", "8L-1", "1024")


def class_limbs(c):
    return 8 << c


def class_edges(c):
    """(lo, hi): the shortest and the longest modulus of class c, in bytes"""
    return (2 * class_limbs(c) + 1 if c else 1), 4 * class_limbs(c)


def width_class(ml):
    return next(c for c in range(NCLASS) if ml <= class_edges(c)[1])


def class_mod_lens(c):
    """every residue mod 4 at both edges of the class"""
    lo, hi = class_edges(c)
    if c in THIN_CLASSES:
        return [lo, hi - 1]
    return [lo, lo + 1, lo + 2, lo + 3, hi - 3, hi - 2, hi - 1, hi]


def base_len(kind, ml):
    L = class_limbs(width_class(ml))
    v = {"0": 0, "1": 1, "ml-1": ml - 1, "ml+1": ml + 1, "4L+1": 4 * L + 1, "8L-1": 8 * L - 1, "1024": 1024}[kind]
    return min(v, 1024)


def class_exp_lens(c):
    return (0, 1, 2) if class_edges(c)[0] >= SMALL_EXP_FROM else (0, 1, 3, 33)


def dev_shapes(c=None):
    """(bl, el, ml) of the launches of class c (of every class in turn for None), without repeats.  Every
    kind of base length meets a non-zero exponent at a modulus length that is no multiple of 4, in turn over
    those lengths; the lengths that are a multiple of 4 get a base one byte longer and one byte shorter;
    el = 0 comes with bl = 0 at the shortest modulus and with a longer base; the 1024-byte exponent field
    comes once, at the length = 3 (mod 4) below the upper edge."""
    if c is None:
        return [s for k in range(NCLASS) for s in dev_shapes(k)]
    mls = class_mod_lens(c)
    ragged = [m for m in mls if m % 4]
    els = [e for e in class_exp_lens(c) if e]
    out = []
    for i, kind in enumerate(BASE_LEN_KINDS):
        ml = ragged[i % len(ragged)]
        out.append((base_len(kind, ml), els[i % len(els)], ml))
    for i, ml in enumerate(m for m in mls if m % 4 == 0):
        out.append((base_len(("ml+1", "ml-1")[i % 2], ml), els[(i + 1) % len(els)], ml))
    out.append((0, 0, ragged[0]))
    out.append((base_len("ml+1", ragged[-2]), 0, ragged[-2]))
    out.append((base_len("ml+1", ragged[-1]), WIDE_EXP_FIELD, ragged[-1]))
    return list(dict.fromkeys(out))


def row_kinds(i):
    """(modulus kind, base kind, exponent kind) of row i of rows(): the modulus kinds turn by lane, so that
    neighbouring lanes of a wave take different paths; the exponent kinds turn by row, one step further every
    seven rows, so that they meet every base kind"""
    return MOD_KINDS[i % len(MOD_KINDS)], BASE_KINDS[i % len(BASE_KINDS)], EXP_KINDS[(i + i // 7) % len(EXP_KINDS)]


def _row(rng, bl, el, ml, mk, bk, ek):
    m = modulus(rng, mk, ml)
    b = base(rng, bk, bl, int.from_bytes(m, "big"))
    if el >= WIDE_EXP_FIELD:
        e = exponent(rng, ek, 2, True).rjust(el, b"\0")
    else:
        e = exponent(rng, ek, el, ml >= SMALL_EXP_FROM)
    return b + e + m


def rows(rng, n, bl, el, ml, start=0):
    """n rows base || exp || mod of one shape, of the kinds row_kinds(start), row_kinds(start + 1), ..."""
    return [_row(rng, bl, el, ml, *row_kinds(start + i)) for i in range(n)]


def model_rows(M, rws, bl, el, ml):
    """the model's outputs of rows of one shape, joined (M is tests/modexp_model.py)"""
    hdr = word(bl) + word(el) + word(ml)
    return b"".join(M.run(hdr + r) for r in rws)


# ---------------------------------------------------------------- the second trip of the grid-stride loop
MAX_WAVES = 2048                  # csrc/modexp_plan.h: a launch of a wide class has at most this many waves
TWO_TRIP_LANES = MAX_WAVES * 64   # the stride of such a launch
TWO_TRIP_FIRST = 128              # rows 0 .. 127: the first items of the lanes of waves 0 and 1
TWO_TRIP_SECOND = 70              # rows TWO_TRIP_LANES .. + 69: the second items of wave 0 and of six lanes of wave 1
TWO_TRIP_N = TWO_TRIP_LANES + TWO_TRIP_SECOND
# the modulus kind of a lane's second item, by the kind of its first (in the order of MOD_KINDS): every pair
# differs in path, an even modulus with k >= 32 meets an odd one or a power of two and the reverse, and the
# zero modulus (which leaves the item before anything is written) comes both before and after an odd one
SECOND_MOD_KINDS = ("zero", "k33", "k32", "2q", "odd", "pow2", "ff", "odd", "pow2", "top0", "k33", "one")
_NONZERO_EXP_KINDS = tuple(k for k in EXP_KINDS if k != "zero")


def two_trip_real():
    """indices of the rows of two_trip_rows() that do work"""
    return list(range(TWO_TRIP_FIRST)) + list(range(TWO_TRIP_LANES, TWO_TRIP_N))


def two_trip_rows(rng, ml, bl, el):
    """(TWO_TRIP_N, bl + el + ml) uint8: the rows of one launch whose waves 0 and 1 come round a second time.
    The rows of two_trip_real() are of the kinds of rows() with non-zero exponents, the second item of a lane
    of the kind SECOND_MOD_KINDS gives; every other row is row TWO_TRIP_FIRST, an odd modulus under an
    all-zero exponent, which the kernel answers with 1 once it has loaded the modulus."""
    import numpy as np
    assert el > 0 and ml > 1

    def real(i, mk):
        _, bk, _ = row_kinds(i)
        ek = _NONZERO_EXP_KINDS[i % len(_NONZERO_EXP_KINDS)]
        r = bytearray(_row(rng, bl, el, ml, mk, bk, ek))
        if not any(r[bl:bl + el]):
            r[bl + el - 1] = 1
        return bytes(r)

    idle = base(rng, "longer", bl, 0) + bytes(el) + modulus(rng, "odd", ml)
    out = np.tile(np.frombuffer(idle, np.uint8), (TWO_TRIP_N, 1))
    for i in range(TWO_TRIP_FIRST):
        out[i] = np.frombuffer(real(i, MOD_KINDS[i % len(MOD_KINDS)]), np.uint8)
    for j in range(TWO_TRIP_SECOND):
        out[TWO_TRIP_LANES + j] = np.frombuffer(real(j + 3, SECOND_MOD_KINDS[j % len(MOD_KINDS)]), np.uint8)
    return out


def two_trip_want(M, arr, bl, el, ml):
    """the model's (TWO_TRIP_N, ml) outputs of two_trip_rows(): the real rows one by one, the idle row once"""
    import numpy as np
    hdr = word(bl) + word(el) + word(ml)
    idle = np.frombuffer(M.run(hdr + arr[TWO_TRIP_FIRST].tobytes()), np.uint8)
    want = np.tile(idle, (TWO_TRIP_N, 1))
    for i in two_trip_real():
        want[i] = np.frombuffer(M.run(hdr + arr[i].tobytes()), np.uint8)
    return want


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
