"""The scalar schedule of the secp256k1 recovery (geth-sharding_amd/csrc/secp256k1_glv.cuh and
secp256k1_comb.cuh, with the constants of secp256k1_dev.cuh) restated in Python integers:
sc_mul_shift272, sc_split_lambda, glv_make_odd, the sign handling, recode_glv, the GLV ladder's add
order and the fixed-base comb's window digits.

Every constant and window width is read from the source text of the device headers, so a change there
flows into the model (or fails the parse); nothing is retyped here.  The model follows the device's
integer widths where they matter (recode_glv keeps five 32-bit limbs, the digit codes keep GLV_W bits).
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "geth-sharding_amd", "csrc")
SOURCES = ("recover_dev.cuh", "gsv_internal.h", "secp256k1_dev.cuh")


def _strip_comments(txt):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


_TEXT = {name: _strip_comments(open(os.path.join(CSRC, name)).read()) for name in SOURCES}


def parse_words(name, nwords=8, text=None):
    """`__device__ constexpr uint32_t NAME[nwords] = {w0, w1, ...};` -> the integer sum w_i 2^(32 i)."""
    hits = []
    for txt in ([text] if text is not None else _TEXT.values()):
        hits += re.findall(r"constexpr\s+uint32_t\s+%s\s*\[\s*(\d+)\s*\]\s*=\s*\{([^}]*)\}\s*;" % re.escape(name), txt)
    if len(hits) != 1:
        raise ValueError("%s: %d definitions found in %s" % (name, len(hits), SOURCES))
    size, body = hits[0]
    words = [w.strip() for w in body.split(",")]
    if int(size) != nwords or len(words) != nwords:
        raise ValueError("%s: %s words declared, %d given, %d expected" % (name, size, len(words), nwords))
    val = 0
    for i, w in enumerate(words):
        m = re.fullmatch(r"(0[xX][0-9a-fA-F]{1,8}|\d+)[uU]?", w)
        if not m:
            raise ValueError("%s: word %d is not a 32-bit literal: %r" % (name, i, w))
        v = int(m.group(1), 0)
        if v >> 32:
            raise ValueError("%s: word %d does not fit 32 bits" % (name, i))
        val |= v << (32 * i)
    return val


def parse_int(name, env=None, text=None):
    """`constexpr int NAME = <integer expression of literals and earlier constants>;`"""
    hits = []
    for txt in ([text] if text is not None else _TEXT.values()):
        hits += re.findall(r"constexpr\s+int\s+%s\s*=\s*([^;]+);" % re.escape(name), txt)
    if len(hits) != 1:
        raise ValueError("%s: %d definitions found in %s" % (name, len(hits), SOURCES))
    expr = hits[0].strip()
    if not re.fullmatch(r"[\w\s()+\-*/<>]+", expr) or "//" in expr:
        raise ValueError("%s: cannot evaluate %r" % (name, expr))
    names = set(re.findall(r"[A-Za-z_]\w*", expr))
    env = dict(env or {})
    missing = names - set(env)
    if missing:
        raise ValueError("%s: %r uses unknown names %s" % (name, expr, sorted(missing)))
    val = eval(expr.replace("/", "//"), {"__builtins__": {}}, env)  # C integer division of positives
    if not isinstance(val, int) or val <= 0:
        raise ValueError("%s: %r evaluated to %r" % (name, expr, val))
    return val


GLV_W = parse_int("GLV_W")
GLV_NT = parse_int("GLV_NT", {"GLV_W": GLV_W})
GLV_DIGITS = parse_int("GLV_DIGITS", {"GLV_W": GLV_W})
COMB_BITS = parse_int("COMB_BITS")
COMB_WINDOWS = parse_int("COMB_WINDOWS", {"COMB_BITS": COMB_BITS})

N = parse_words("SN")
HALF_N = parse_words("HALF_N")
MINUS_LAMBDA = parse_words("MINUS_LAMBDA")
MINUS_B1 = parse_words("MINUS_B1")
MINUS_B2 = parse_words("MINUS_B2")
GLV_G1 = parse_words("GLV_G1")
GLV_G2 = parse_words("GLV_G2")
GLV_V1A = parse_words("GLV_V1A")
GLV_V1B = parse_words("GLV_V1B")
GLV_V2A = parse_words("GLV_V2A")
GLV_V3A = parse_words("GLV_V3A")
GLV_V3B = parse_words("GLV_V3B")
BETA = parse_words("BETA")
P = parse_words("FP")
GX = parse_words("GX")
GY = parse_words("GY")
LAMBDA = N - MINUS_LAMBDA
GLV_V = {"V1A": GLV_V1A, "V1B": GLV_V1B, "V2A": GLV_V2A, "V3A": GLV_V3A, "V3B": GLV_V3B}
# the lattice vectors glv_make_odd adds, by branch: (to k1, to k2)
BRANCH_VECTORS = {"v1": (GLV_V1A, GLV_V1B), "v2": (GLV_V2A, GLV_V1A), "v3": (GLV_V3A, GLV_V3B), "none": (0, 0)}


def signed(k):
    """the representative of k mod n in (-n/2, n/2]"""
    k %= N
    return k - N if k > HALF_N else k


# ---------------------------------------------------------------- the scalar schedule
def mul_shift272(k, g):
    """sc_mul_shift272: (k g) >> 272, rounded by bit 271 of the 512-bit product"""
    t = k * g
    return ((t >> 272) + ((t >> 271) & 1)) & ((1 << 256) - 1)


def split_lambda(k):
    """sc_split_lambda: (r1, r2) mod n with r1 + r2 lambda == k"""
    c1 = mul_shift272(k, GLV_G1) * MINUS_B1 % N
    c2 = mul_shift272(k, GLV_G2) * MINUS_B2 % N
    r2 = (c1 + c2) % N
    r1 = (r2 * MINUS_LAMBDA + k) % N
    return r1, r2


def is_high(a):
    return a > HALF_N


def make_odd(k1, k2):
    """glv_make_odd: (k1, k2, branch) with branch in v1 / v2 / v3 / none"""
    odd1 = ((k1 & 1) != 0) != is_high(k1)
    odd2 = ((k2 & 1) != 0) != is_high(k2)
    branch = "v1" if (not odd1 and not odd2) else "v2" if (odd1 and not odd2) else \
        "v3" if (not odd1 and odd2) else "none"
    a, b = BRANCH_VECTORS[branch]
    return (k1 + a) % N, (k2 + b) % N, branch


def magnitude(k):
    """recover_core's sign handling: (negative, |k|)"""
    neg = is_high(k)
    return neg, (N - k) % N if neg else k


def recode(mag):
    """recode_glv on the low five 32-bit limbs of mag.  Returns (skew, codes, digits, rest): codes are
    the GLV_W-bit digit codes the device packs (sign bit above a table index), digits the signed
    values recode_glv computed, rest what is left of k after the last digit (0 when the digits hold
    all of k)."""
    mask, off, m160 = (2 << GLV_W) - 1, 1 << GLV_W, (1 << 160) - 1
    k = mag & m160
    skew = (k & 1) ^ 1
    k = (k + skew) & m160
    digits = []
    for i in range(GLV_DIGITS):
        d = (k & mask) - off if i < GLV_DIGITS - 1 else (k & mask)
        digits.append(d)
        k = ((k - d) & m160) >> GLV_W
    codes = [((d < 0) << (GLV_W - 1)) | (((abs(d) - 1) & 0xFFFFFFFF) >> 1) for d in digits]
    return skew, codes, digits, k


def decode(code):
    """what the ladder makes of a digit code: the sign bit and the table index, as a signed odd digit
    (bits of the code above the sign bit would run into the next digit's slot: reported as None)"""
    if code >> GLV_W:
        return None
    d = 2 * (code & (GLV_NT - 1)) + 1
    return -d if code >> (GLV_W - 1) else d


_DECODE = {c: decode(c) for c in range(1 << GLV_W)}


class Schedule:
    """everything recover_core derives from u2 before the ladder runs"""

    def __init__(self, u2):
        self.u2 = u2
        self.split = split_lambda(u2)
        k1, k2, self.branch = make_odd(*self.split)
        self.k = (k1, k2)
        (self.neg1, self.mag1), (self.neg2, self.mag2) = magnitude(k1), magnitude(k2)
        self.skew1, self.codes1, self.digits1, self.rest1 = recode(self.mag1)
        self.skew2, self.codes2, self.digits2, self.rest2 = recode(self.mag2)


# the addends' scalars by pass and signed digit: d on T, d lambda on lambda T
_ADDEND = [{d: (d * f) % N for d in range(1 - 2 * GLV_NT, 2 * GLV_NT, 2)} for f in (1, LAMBDA)]


def ladder(s: Schedule):
    """The ladder's running scalar (acc = running * R).  Order as in recover_core: digit GLV_DIGITS-1
    down to 0, GLV_W doublings before every digit but the first, pass j = 0 adds the k1 digit on T,
    pass j = 1 the k2 digit on lambda T; the first pass of the top digit starts the sum.
    Returns (final running scalar, events): events are (kind, digit index, pass) with kind "dbl" (the
    accumulator equals the addend: the mixed add's doubling), "inf" (it equals minus the addend: the sum
    is the identity) and "identity" (the accumulator is the identity when the add starts)."""
    run = None
    events = []
    top = GLV_DIGITS - 1
    codes, negs = (s.codes1, s.codes2), (s.neg1, s.neg2)
    for i in range(top, -1, -1):
        if i != top:
            run = (run << GLV_W) % N
        for j in (0, 1):
            d = _DECODE.get(codes[j][i])
            if d is None:
                raise ValueError("digit code wider than GLV_W bits at digit %d, pass %d" % (i, j))
            add = _ADDEND[j][-d if negs[j] else d]
            if run is None:
                run = add
                continue
            if run == add:
                events.append(("dbl", i, j))
            elif run == 0:
                events.append(("identity", i, j))
            run += add
            if run >= N:
                run -= N
                if run == 0:
                    events.append(("inf", i, j))
    return run, events


def comb_digits(u):
    """comb_mul_g9's window digits: entry (w, d_w) = d_w 2^(COMB_BITS w) G is read for every w"""
    return [(u >> (COMB_BITS * w)) & ((1 << COMB_BITS) - 1) for w in range(COMB_WINDOWS)]


# ---------------------------------------------------------------- the families of scalars under test
def small_family(bound):
    """a + b lambda mod n for |a|, |b| <= bound, without 0: [(u2, a, b)]"""
    return [((a + b * LAMBDA) % N, a, b) for a in range(-bound, bound + 1) for b in range(-bound, bound + 1)
            if (a, b) != (0, 0)]


def near_constant_centres():
    """the values the near-constant family surrounds: [(name, centre)]"""
    c = [("n-1", N - 1), ("n/2", N // 2), ("2^128", 1 << 128), ("2^129", 1 << 129), ("lambda", LAMBDA),
         ("-lambda", N - LAMBDA)]
    for name, v in sorted(GLV_V.items()):
        c += [(name, v), ("-" + name, N - v)]
    for m in (3, 5, 7, 9, 11, 13, 128):
        c += [("%d n/%d" % (t, m), t * N // m) for t in range(1, m)]
    return c


def near_constant_family(radius=50):
    """centre + e mod n for |e| <= radius around every centre, without 0 and without repeats: [u2]"""
    seen, out = set(), []
    for _, c in near_constant_centres():
        for e in range(-radius, radius + 1):
            u = (c + e) % N
            if u and u not in seen:
                seen.add(u)
                out.append(u)
    return out


def family(key):
    """the two structured families by name: "small" (|a|, |b| <= 150) and "near" (the near-constant one)"""
    if key == "small":
        return [u for u, _, _ in small_family(150)]
    if key == "near":
        return near_constant_family()
    raise KeyError(key)


_WALKS = {}


def walk(scalars, check=None):
    """Schedule and ladder of every scalar.  Returns (events {u2: ladder events}, wrong [u2 whose final
    running scalar is not u2], branches {branch: count}); check(schedule), if given, sees every schedule."""
    events, wrong, branches = {}, [], dict.fromkeys(BRANCH_VECTORS, 0)
    for u in scalars:
        s = Schedule(u)
        if check is not None:
            check(s)
        run, ev = ladder(s)
        if run != u:
            wrong.append(u)
        if ev:
            events[u] = ev
        branches[s.branch] += 1
    return events, wrong, branches


def walk_family(key, check=None):
    """walk(family(key)), computed once per process (again when a check is to see the schedules)"""
    if check is not None or key not in _WALKS:
        _WALKS[key] = walk(family(key), check)
    return _WALKS[key]


def exceptional_scalars():
    """{u2: events}: the scalars of the two structured families whose ladder meets a doubling ("dbl"),
    a sum that is the identity ("inf") or an identity accumulator ("identity")"""
    out = {}
    for key in ("small", "near"):
        out.update(walk_family(key)[0])
    return out


# ---------------------------------------------------------------- affine arithmetic, Python integers
def ec_add(a, b):
    """a + b on y^2 = x^3 + 7 over F_p; None is the identity"""
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        l = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else:
        l = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (l * l - a[0] - b[0]) % P
    return x, (l * (a[0] - x) - a[1]) % P


def ec_mul(k, pt):
    k %= N
    acc = None
    while k:
        if k & 1:
            acc = ec_add(acc, pt)
        pt = ec_add(pt, pt)
        k >>= 1
    return acc


G = (GX, GY)


def lift_x(x, odd):
    """the curve point with this x and y of the given parity, or None"""
    if not 0 <= x < P:
        return None
    c = (x * x * x + 7) % P
    y = pow(c, (P + 1) // 4, P)
    if y * y % P != c:
        return None
    return x, y if (y & 1) == odd else P - y


def craft(R, u1, u2):
    """(msg, r, s, recid) whose recovery computes u1 G + u2 R: r = x_R (< n), s = u2 r, msg = -u1 r"""
    assert R[0] < N and u2 % N
    r = R[0]
    return (-u1 * r) % N, r, u2 * r % N, R[1] & 1


def recover_expected(R, u1, u2):
    """u1 G + u2 R in affine Python integers (None: the identity, recovery fails)"""
    return ec_add(ec_mul(u1, G), ec_mul(u2, R))
