"""Generates geth-sharding_amd/csrc/fe9_asm.cuh: secp256k1_fe9.cuh's fe9_mul / fe9_sqr (9 x 29-bit
column product + the 2^261 == 2^37 + 31264 fold of fe9_reduce) as ONE inline-asm statement each.

Why asm.  Written as C++ (`acc += (uint64_t)a[i] * b[j]` per term, `acc >>= 29` per column),
LLVM re-associates each column's sum into a v_mad_u64_u32 chain that starts at 0 and adds the
incoming carry with a separate v_lshl_add_u64 (17 extra 64-bit VALU ops per product, 8 more in
the reduction).  Pinning the order with an empty asm after every multiply-add removes those, but
hipcc then pads a wait state (s_nop 0) after every asm boundary whose output the next VALU reads:
73 per product.  One statement for the whole operation has neither: column k's accumulator
starts as the previous column shifted right by 29 (v_lshrrev_b64) and takes its products as one
chain; the reduction's running value keeps its carry in a register pair whose high word is 0.

Inline asm cannot name the low half of a 64-bit operand, so the two running pairs live in fixed,
clobbered VGPRs (v[2:3], v[4:5]) and the 29-bit limbs are read from their low registers.
full_lines() is also executed instruction by instruction by tests/test_asm_emulated.py."""
import os

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "geth-sharding_amd", "csrc", "fe9_asm.cuh")


def full(name, doc, terms_of_column, addend=False, dot=False):
    L = full_lines(terms_of_column, addend)
    outs = ", ".join([f'"=&v"(r[{i}])' for i in range(9)] + [f'"=&v"(hi[{i}])' for i in range(8)] + ['"=&s"(sd)'])
    ins = ", ".join([f'"v"(a[{i}])' for i in range(9)] + [f'"v"(b[{j}])' for j in range(9)] +
                    ['"s"(k31264)', '"s"(k256)', '"s"(k977)'] +
                    ([f'"v"(c[{j}])' for j in range(9)] if addend or dot else []) +
                    ([f'"v"(d[{j}])' for j in range(9)] if dot else []))
    body = "\\n\\t".join(L)
    return [f"// {doc}",
            f"__device__ __forceinline__ void {name}(uint32_t r[9], const uint32_t a[9], const uint32_t b[9]"
            + (", const uint32_t c[9]" if addend or dot else "") + (", const uint32_t d[9]" if dot else "") + ") {",
            "    uint32_t hi[8];",
            "    uint64_t sd;",
            "    uint32_t k31264 = 31264u, k256 = 256u, k977 = 977u;",
            f'    asm("{body}"',
            f"        : {outs}",
            f"        : {ins}",
            '        : "v2", "v3", "v4", "v5");',
            "}"]


MUL_TERMS = lambda k: [(i, 9 + (k - i)) for i in range(9) if 0 <= k - i < 9]


def DOT_TERMS(k):
    """a b + c d: both products' terms in one column chain (one reduction for the two)"""
    return MUL_TERMS(k) + [(18 + i, 27 + (k - i)) for i in range(9) if 0 <= k - i < 9]


def SQR_TERMS(k):
    """squaring: b holds the doubled limbs 2 a[j]; cross terms a[i] * 2a[j] (i < j) + a[k/2]^2"""
    t = [(i, 9 + (k - i)) for i in range(9) if i < k - i < 9]
    if k % 2 == 0 and k // 2 < 9:
        t.append((k // 2, k // 2))
    return t


def DOT_MS_TERMS(k):
    """a b + c^2 with d = 2c limb-wise (fe9_dot_ms: the W doubling's -W3 = E 2(X3 - D) + B B): the
    product's 81 terms, the squaring's cross terms c[i] * d[j] (i < j) and its diagonal c[k/2]^2 in one
    column chain, one reduction.  Bound m_a m_b + m_c^2 <= 7: a column's terms sum to < 63 2^58, as
    for fe9_mul."""
    t = MUL_TERMS(k) + [(18 + i, 27 + (k - i)) for i in range(9) if i < k - i < 9]
    if k % 2 == 0 and k // 2 < 9:
        t.append((18 + k // 2, 18 + k // 2))
    return t


def SQR3_TERMS(k):
    """3 a^2 with b = 6a and c = 3a limb-wise (fe9_sqr3: the doubling's E = 3 X^2): cross terms
    a[i] * 6a[j] (i < j) + a[k/2] * 3a[k/2].  Bound m_a <= 1.33 (6a fits 32 bits; 3 m_a^2 <= 5.4): the
    multiply-by-3 of a reduced square and its normalisation become part of the squaring."""
    t = [(i, 9 + (k - i)) for i in range(9) if i < k - i < 9]
    if k % 2 == 0 and k // 2 < 9:
        t.append((k // 2, 18 + k // 2))
    return t


def full_lines(terms_of_column, addend=False):
    """Product + reduction (secp256k1_fe9.cuh fe9_reduce restated) in one statement.  Operands:
    %0..%8 r (o_0..o_8 in place), %9..%16 o_9..o_16, %17 sd, %18..%26 a, %27..%35 b,
    %36 31264, %37 256, %38 977 (SGPRs), with `addend` %39..%47 the limbs of c (each < 2^31),
    added to o_0..o_8 as the reduction reads them (r = a b + c; the 32-bit add that takes o_j becomes
    a three-operand add, no further instruction).  Fixed pairs: C = v[2:3] (columns, then o17, then
    T), D = v[4:5] (the reduction's running value)."""
    cj = lambda j: f"%{39 + j}"
    # term operand numbering: 0..8 a, 9..17 b, 18..26 c (%39..), 27..35 d (%48..; fe9_dot only)
    opnd = lambda x: f"%{18 + x}" if x < 18 else f"%{39 + (x - 18)}"
    C, c0, c1 = "v[2:3]", "v2", "v3"
    D, d0, d1 = "v[4:5]", "v4", "v5"
    o = lambda k: f"%{k}" if k < 9 else f"%{k}"
    a = lambda i: f"%{18 + i}"
    b = lambda j: f"%{27 + j}"
    K31264, K256, K977, SD = "%36", "%37", "%38", "%17"
    L = []
    for k in range(17):
        first = True
        if k > 0:
            L.append(f"v_lshrrev_b64 {C}, 29, {C}")
            first = False
        for (x, y) in terms_of_column(k):
            L.append(f"v_mad_u64_u32 {C}, {SD}, {opnd(x)}, {opnd(y)}, {'0' if first else C}")
            first = False
        L.append(f"v_and_b32_e32 {o(k)}, 0x1fffffff, {c0}")
    L.append(f"v_lshrrev_b64 {C}, 29, {C}")               # o17 < 2^35
    # limbs 0..7: c = o_j + carry + 31264 o_{j+9} + 256 o_{j+8}
    L.append(f"v_mov_b32 {d1}, 0")
    if addend:
        L.append(f"v_add_u32 {d0}, {o(0)}, {cj(0)}")       # o_0 + c_0 < 2^29 + 2^31
    else:
        L.append(f"v_mov_b32 {d0}, {o(0)}")
    L.append(f"v_mad_u64_u32 {D}, {SD}, {o(9)}, {K31264}, {D}")
    L.append(f"v_and_b32_e32 {o(0)}, 0x1fffffff, {d0}")
    for j in range(1, 8):
        L.append(f"v_lshrrev_b64 {D}, 29, {D}")           # carry < 2^17: the high word is 0
        if addend:
            L.append(f"v_add3_u32 {d0}, {d0}, {o(j)}, {cj(j)}")
        else:
            L.append(f"v_add_u32 {d0}, {d0}, {o(j)}")
        L.append(f"v_mad_u64_u32 {D}, {SD}, {o(j + 9)}, {K31264}, {D}")
        L.append(f"v_mad_u64_u32 {D}, {SD}, {o(j + 8)}, {K256}, {D}")
        L.append(f"v_and_b32_e32 {o(j)}, 0x1fffffff, {d0}")
    # limb 8: o_8 + carry + 31264 o17 + 256 o_16; 24 bits stay, the rest (units of 2^256) is T
    L.append(f"v_lshrrev_b64 {D}, 29, {D}")
    if addend:
        L.append(f"v_add3_u32 {d0}, {d0}, {o(8)}, {cj(8)}")
    else:
        L.append(f"v_add_u32 {d0}, {d0}, {o(8)}")
    L.append(f"v_mad_u64_u32 {D}, {SD}, {c0}, {K31264}, {D}")
    L.append(f"v_mad_u32_u24 {d1}, {c1}, {K31264}, {d1}")
    L.append(f"v_mad_u64_u32 {D}, {SD}, {o(16)}, {K256}, {D}")
    L.append(f"v_and_b32_e32 {o(8)}, 0xffffff, {d0}")
    L.append(f"v_lshrrev_b64 {D}, 24, {D}")
    L.append(f"v_lshlrev_b64 {C}, 13, {C}")             # (v_lshl_add_u64 shifts by 0..4 only)
    L.append(f"v_lshl_add_u64 {C}, {C}, 0, {D}")        # T = (c >> 24) + (o17 << 13) < 2^49
    # 2^256 == 2^32 + 977: limb 0 += 977 T, limb 1 += 8 T (+ carries), limb 2 += carry
    L.append(f"v_mov_b32 {d1}, 0")
    L.append(f"v_mov_b32 {d0}, {o(0)}")
    L.append(f"v_mad_u64_u32 {D}, {SD}, {c0}, {K977}, {D}")
    L.append(f"v_mad_u32_u24 {d1}, {c1}, {K977}, {d1}")
    L.append(f"v_and_b32_e32 {o(0)}, 0x1fffffff, {d0}")
    L.append(f"v_lshrrev_b64 {D}, 29, {D}")
    L.append(f"v_lshl_add_u64 {D}, {C}, 3, {D}")
    L.append(f"v_mad_u64_u32 {D}, {SD}, {o(1)}, 1, {D}")
    L.append(f"v_and_b32_e32 {o(1)}, 0x1fffffff, {d0}")
    L.append(f"v_alignbit_b32 {c0}, {d1}, {d0}, 29")
    L.append(f"v_add_u32 {o(2)}, {o(2)}, {c0}")
    return L



# ---------------------------------------------------------------------------- column form 2
# Operand numbering of the form-2 statements (the emulator test reads it): %0..%8 r, %9 the dead
# carry-out SGPR pair, then a, b, the three SGPR constants, c, d.
OPND2 = {"r": 0, "sd": 9, "a": 10, "b": 19, "k31264": 28, "k256": 29, "k977": 30, "k8192": 31, "c": 32, "d": 41}
PAIR2 = {k: f"v[{6 + 2 * (k - 10)}:{7 + 2 * (k - 10)}]" for k in range(10, 17)}  # columns 10..16


def full_lines2(terms_of_column, addend=False):
    """Form 2: the high columns 9..16 are never masked or shifted.  Column 9 accumulates in
    C = v[2:3] (from column 8's C >> 29, as form 1); column k = 10..16 in its own fixed pair P_k
    (v[6:7] .. v[18:19]) starting from 8 * hi(P_{k-1}) (one multiply-add, in place of the 64-bit shift)
    and keeps its 32-bit low word o_k = C_k mod 2^32 unmasked: sum_k o_k 2^(29 k) is still the product,
    because the carry into column k is floor(C_{k-1} / 2^32) at weight 2^(29 (k-1) + 32) = 8 * 2^(29 k).
    The reduction reads o_9..o_16 through multiply-adds (31264 o, 256 o < 2^47), so an unmasked 32-bit
    limb costs nothing there; o17 = 8 hi(P_16) < 2^23 is a 32-bit value (one shift), and
    T = (c >> 24) + o17 2^13 one multiply-add.  Per product 8 masks, a 64-bit shift, a 64-bit
    shift-add and a u24 multiply-add fewer than form 1."""
    O = OPND2
    opnd = lambda x: f"%{O['a'] + x}" if x < 9 else (f"%{O['b'] + x - 9}" if x < 18 else f"%{O['c'] + x - 18}")
    cj = lambda j: f"%{O['c'] + j}"
    r = lambda k: f"%{O['r'] + k}"
    C, c0, c1 = "v[2:3]", "v2", "v3"
    D, d0, d1 = "v[4:5]", "v4", "v5"
    lo = lambda k: "v2" if k == 9 else f"v{6 + 2 * (k - 10)}"
    hi = lambda k: "v3" if k == 9 else f"v{7 + 2 * (k - 10)}"
    K31264, K256, K977, SD = f"%{O['k31264']}", f"%{O['k256']}", f"%{O['k977']}", f"%{O['sd']}"
    K8192 = f"%{O['k8192']}"  # VOP3 takes no literal on gfx950: 2^13 from an SGPR
    L = []
    for k in range(17):
        if k <= 9:
            acc, first = C, True
            if k > 0:
                L.append(f"v_lshrrev_b64 {C}, 29, {C}")
                first = False
        else:
            acc = PAIR2[k]
            L.append(f"v_mad_u64_u32 {acc}, {SD}, {hi(k - 1)}, 8, 0")  # 8 * floor(C_{k-1} / 2^32)
            first = False
        for (x, y) in terms_of_column(k):
            L.append(f"v_mad_u64_u32 {acc}, {SD}, {opnd(x)}, {opnd(y)}, {'0' if first else acc}")
            first = False
        if k <= 8:
            L.append(f"v_and_b32_e32 {r(k)}, 0x1fffffff, {c0}")
    L.append(f"v_lshlrev_b32 {c1}, 3, {hi(16)}")          # o17 = 8 hi(P_16) (C's high word is free)
    # limbs 0..7: c = o_j + carry + 31264 o_{j+9} + 256 o_{j+8}
    L.append(f"v_mov_b32 {d1}, 0")
    if addend:
        L.append(f"v_add_u32 {d0}, {r(0)}, {cj(0)}")
    else:
        L.append(f"v_mov_b32 {d0}, {r(0)}")
    L.append(f"v_mad_u64_u32 {D}, {SD}, {lo(9)}, {K31264}, {D}")
    L.append(f"v_and_b32_e32 {r(0)}, 0x1fffffff, {d0}")
    for j in range(1, 8):
        L.append(f"v_lshrrev_b64 {D}, 29, {D}")           # carry < 2^19: the high word is 0
        if addend:
            L.append(f"v_add3_u32 {d0}, {d0}, {r(j)}, {cj(j)}")
        else:
            L.append(f"v_add_u32 {d0}, {d0}, {r(j)}")
        L.append(f"v_mad_u64_u32 {D}, {SD}, {lo(j + 9)}, {K31264}, {D}")
        L.append(f"v_mad_u64_u32 {D}, {SD}, {lo(j + 8)}, {K256}, {D}")
        L.append(f"v_and_b32_e32 {r(j)}, 0x1fffffff, {d0}")
    # limb 8: o_8 + carry + 31264 o17 + 256 o_16; 24 bits stay, the rest (units of 2^256) is T
    L.append(f"v_lshrrev_b64 {D}, 29, {D}")
    if addend:
        L.append(f"v_add3_u32 {d0}, {d0}, {r(8)}, {cj(8)}")
    else:
        L.append(f"v_add_u32 {d0}, {d0}, {r(8)}")
    L.append(f"v_mad_u64_u32 {D}, {SD}, {c1}, {K31264}, {D}")
    L.append(f"v_mad_u64_u32 {D}, {SD}, {lo(16)}, {K256}, {D}")
    L.append(f"v_and_b32_e32 {r(8)}, 0xffffff, {d0}")
    L.append(f"v_lshrrev_b64 {D}, 24, {D}")
    T, t0, t1 = "v[6:7]", "v6", "v7"                      # P_10 is dead by now
    L.append(f"v_mad_u64_u32 {T}, {SD}, {c1}, {K8192}, {D}")  # T = (c >> 24) + o17 2^13 < 2^37
    # 2^256 == 2^32 + 977: limb 0 += 977 T, limb 1 += 8 T (+ carries), limb 2 += carry
    L.append(f"v_mov_b32 {d1}, 0")
    L.append(f"v_mov_b32 {d0}, {r(0)}")
    L.append(f"v_mad_u64_u32 {D}, {SD}, {t0}, {K977}, {D}")
    L.append(f"v_mad_u32_u24 {d1}, {t1}, {K977}, {d1}")
    L.append(f"v_and_b32_e32 {r(0)}, 0x1fffffff, {d0}")
    L.append(f"v_lshrrev_b64 {D}, 29, {D}")
    L.append(f"v_lshl_add_u64 {D}, {T}, 3, {D}")
    L.append(f"v_mad_u64_u32 {D}, {SD}, {r(1)}, 1, {D}")
    L.append(f"v_and_b32_e32 {r(1)}, 0x1fffffff, {d0}")
    L.append(f"v_alignbit_b32 {t0}, {d1}, {d0}, 29")
    L.append(f"v_add_u32 {r(2)}, {r(2)}, {t0}")
    return L


# ---------------------------------------------------------------------------- column form 3
# 1: the high columns emitted round-robin across their independent chains (measured equal at two
# waves per SIMD, profiles/r04/ab/il_*.json: the other wave already hides the chains' latency)
INTERLEAVE3 = os.environ.get("GSV_FE9_INTERLEAVE", "0") == "1"

def full_lines3(terms_of_column, addend=False):
    """Form 3: form 2's high columns, computed FIRST (column 9 from 0 instead of column 8's carry),
    and the low columns 0..8 never carried on their own: limb j's running value is the reduction's
    carry + column j's products + 31264 o_{j+9} + 256 o_{j+8} (+ c_j), one 64-bit multiply-add chain,
    then one mask and one 64-bit shift.  Form 2 carried every low column (shift + mask) and then ran
    the reduction's own carry chain over the masked limbs (a 32-bit add, a mask and a shift again):
    per product 9 64-bit shifts, 9 masks and 9 adds fewer.  Bounds: a column's products sum to
    < 63 2^58 (the m_a m_b <= 7 precondition), the carry is < 2^35, the folds < 2^47 + 2^40 and the
    addend < 2^31: < 2^64.  Limb 8's remainder c >> 24 < 2^40 and o17 < 2^32 make T < 2^46.  With an
    addend, c_j enters as one multiply-add by 1 (the three-operand add of form 2 is gone with the
    separate column carry)."""
    O = OPND2
    opnd = lambda x: f"%{O['a'] + x}" if x < 9 else (f"%{O['b'] + x - 9}" if x < 18 else f"%{O['c'] + x - 18}")
    cj = lambda j: f"%{O['c'] + j}"
    r = lambda k: f"%{O['r'] + k}"
    C, c0, c1 = "v[2:3]", "v2", "v3"
    D, d0, d1 = "v[4:5]", "v4", "v5"
    lo = lambda k: "v2" if k == 9 else f"v{6 + 2 * (k - 10)}"
    hi = lambda k: "v3" if k == 9 else f"v{7 + 2 * (k - 10)}"
    K31264, K256, K977, SD = f"%{O['k31264']}", f"%{O['k256']}", f"%{O['k977']}", f"%{O['sd']}"
    K8192 = f"%{O['k8192']}"
    L = []
    acc_of = lambda k: C if k == 9 else PAIR2[k]
    if INTERLEAVE3:
        # the eight high columns' product chains are independent: emitted round-robin (one term of
        # each column in turn), each from 0; the carries 8 hi(P_{k-1}) follow as one short chain
        cols = {k: list(terms_of_column(k)) for k in range(9, 17)}
        for t in range(max(len(v) for v in cols.values())):
            for k in range(9, 17):
                if t < len(cols[k]):
                    x, y = cols[k][t]
                    acc = acc_of(k)
                    L.append(f"v_mad_u64_u32 {acc}, {SD}, {opnd(x)}, {opnd(y)}, {'0' if t == 0 else acc}")
        for k in range(10, 17):
            acc = acc_of(k)
            L.append(f"v_mad_u64_u32 {acc}, {SD}, {hi(k - 1)}, 8, {acc if cols[k] else '0'}")
    else:
        for k in range(9, 17):                             # high columns: form 2's chains
            if k == 9:
                acc, first = C, True
            else:
                acc = PAIR2[k]
                L.append(f"v_mad_u64_u32 {acc}, {SD}, {hi(k - 1)}, 8, 0")
                first = False
            for (x, y) in terms_of_column(k):
                L.append(f"v_mad_u64_u32 {acc}, {SD}, {opnd(x)}, {opnd(y)}, {'0' if first else acc}")
                first = False
    L.append(f"v_lshlrev_b32 {c1}, 3, {hi(16)}")           # o17 = 8 hi(P_16) < 2^32
    for j in range(9):                                     # low limbs: products + folds, one carry
        first = j == 0
        if addend:
            L.append(f"v_mad_u64_u32 {D}, {SD}, {cj(j)}, 1, {'0' if first else D}")
            first = False
        for (x, y) in terms_of_column(j):
            L.append(f"v_mad_u64_u32 {D}, {SD}, {opnd(x)}, {opnd(y)}, {'0' if first else D}")
            first = False
        if j < 8:
            L.append(f"v_mad_u64_u32 {D}, {SD}, {lo(j + 9)}, {K31264}, {D}")
            if j:
                L.append(f"v_mad_u64_u32 {D}, {SD}, {lo(j + 8)}, {K256}, {D}")
            L.append(f"v_and_b32_e32 {r(j)}, 0x1fffffff, {d0}")
            L.append(f"v_lshrrev_b64 {D}, 29, {D}")       # carry < 2^35
        else:
            L.append(f"v_mad_u64_u32 {D}, {SD}, {c1}, {K31264}, {D}")
            L.append(f"v_mad_u64_u32 {D}, {SD}, {lo(16)}, {K256}, {D}")
            L.append(f"v_and_b32_e32 {r(8)}, 0xffffff, {d0}")
            L.append(f"v_lshrrev_b64 {D}, 24, {D}")
    T, t0, t1 = "v[6:7]", "v6", "v7"                      # P_10 is dead by now
    L.append(f"v_mad_u64_u32 {T}, {SD}, {c1}, {K8192}, {D}")  # T = (c >> 24) + o17 2^13 < 2^46
    L.append(f"v_mov_b32 {d1}, 0")
    L.append(f"v_mov_b32 {d0}, {r(0)}")
    L.append(f"v_mad_u64_u32 {D}, {SD}, {t0}, {K977}, {D}")
    L.append(f"v_mad_u32_u24 {d1}, {t1}, {K977}, {d1}")
    L.append(f"v_and_b32_e32 {r(0)}, 0x1fffffff, {d0}")
    L.append(f"v_lshrrev_b64 {D}, 29, {D}")
    L.append(f"v_lshl_add_u64 {D}, {T}, 3, {D}")
    L.append(f"v_mad_u64_u32 {D}, {SD}, {r(1)}, 1, {D}")
    L.append(f"v_and_b32_e32 {r(1)}, 0x1fffffff, {d0}")
    L.append(f"v_alignbit_b32 {t0}, {d1}, {d0}, 29")
    L.append(f"v_add_u32 {r(2)}, {r(2)}, {t0}")
    return L


# ------------------------------------------------------- column form 3 with subtrahends
# K p is added so that the value stays non-negative: -K (2^32 + 977) starts limb 0's chain, +K joins
# T (units of 2^256)
SUB_K = 8192
SUB_BIAS0 = -SUB_K * ((1 << 32) + 977)


def opnd3s(nsub):
    """Operand numbering of the subtrahend statements: form 2's, then the subtrahend arrays (9 limbs
    each), the 64-bit SGPR constant SUB_BIAS0 and the SGPR constant 8 * 31264."""
    O = {k: v for k, v in OPND2.items() if k not in ("c", "d")}
    for n in range(nsub):
        O[f"s{n}"] = 32 + 9 * n
    O["kbias"] = 32 + 9 * nsub
    O["k250112"] = 33 + 9 * nsub
    return O


def full_lines3s(terms_of_column, subs):
    """Form 3 with subtrahends: r = (the product the terms spell) - sum_n k_n s_n, for subs = the list
    of k_n in {1, 2} (one 9-limb operand array s_n each).  Limb j of s_n enters limb j's chain as ONE
    v_mad_i64_i32 by the inline constant -k_n, where form 3's addend entered as a multiply-add by 1:
    nothing is negated or biased limb by limb outside the statement.  The low chains D are then SIGNED
    64-bit values: their carries are arithmetic shifts (floor division: D = (D & mask) + 2^29 (D >> 29)
    holds for negative D too), the masks stay, and the unsigned multiply-adds that follow on D are the
    same additions mod 2^64.  The high columns 9..16 hold products only and stay unsigned.

    Bounds (checked instruction by instruction in tests/test_asm_emulated_signed.py).
      * Every s_n limb < 2^31 (the addend's precondition: a non-negative i32).
      * m_a m_b <= 3.5 (squarings: m_a <= 1.87), half of the unsigned forms' 7: a column's products sum
        to < 31.5 2^58, and with the carry (< 2^35) and the folds (< 2^48) a chain stays below 2^63.
        (Z3 = (Z1 + H)^2 - Z1^2 - H^2 squares a magnitude-2 operand, whose column 7 reaches 2^63 + 2^56:
        it keeps the unsigned addend form.)
      * From below: a chain takes at most 3 (2^31 - 1) off (k_0 + k_1 <= 3) and a carry >= -2^17 (limb
        0 starts at SUB_BIAS0 > -2^46): every chain > -2^47.
      * Non-negativity.  The masked limbs are non-negative whatever the chains' signs; what must not be
        negative is T, the part at and above 2^256, which the final fold multiplies as an unsigned
        value.  Limb 8's chain is >= -3 (2^31 - 1) - 2^6, so its carry (>> 24) is >= -385, and
        T = carry + 2^13 o17 + K >= 0 for K = SUB_K = 8192 > 385.  K p = K 2^256 - K (2^32 + 977): the
        second part is limb 0's start, SUB_BIAS0, read from an SGPR pair in the slot where the unsigned
        forms start from 0; the first rides in T's multiply-add as (o17 + 1) 2^13, with o17 + 1 =
        8 hi(P_16) + 1 one v_lshl_add_u32 in place of form 3's shift (limb 8 reads 31264 o17 as
        hi(P_16) * 250112 instead).  No instruction more than the addend form has per subtrahend.
      * T < 2^46 + 2^13, as form 3: the output is a product's output (limb 2 < 2^29 + 2^24)."""
    O = opnd3s(len(subs))
    opnd = lambda x: f"%{O['a'] + x}" if x < 9 else f"%{O['b'] + x - 9}"
    r = lambda k: f"%{O['r'] + k}"
    C, c0, c1 = "v[2:3]", "v2", "v3"
    D, d0, d1 = "v[4:5]", "v4", "v5"
    lo = lambda k: "v2" if k == 9 else f"v{6 + 2 * (k - 10)}"
    hi = lambda k: "v3" if k == 9 else f"v{7 + 2 * (k - 10)}"
    K31264, K256, K977, SD = f"%{O['k31264']}", f"%{O['k256']}", f"%{O['k977']}", f"%{O['sd']}"
    K8192, KBIAS, K250112 = f"%{O['k8192']}", f"%{O['kbias']}", f"%{O['k250112']}"
    L = []
    for k in range(9, 17):                                 # high columns: form 2's chains, unsigned
        if k == 9:
            acc, first = C, True
        else:
            acc = PAIR2[k]
            L.append(f"v_mad_u64_u32 {acc}, {SD}, {hi(k - 1)}, 8, 0")
            first = False
        for (x, y) in terms_of_column(k):
            assert x < 18 and y < 18
            L.append(f"v_mad_u64_u32 {acc}, {SD}, {opnd(x)}, {opnd(y)}, {'0' if first else acc}")
            first = False
    L.append(f"v_lshl_add_u32 {c1}, {hi(16)}, 3, 1")       # o17 + 1 = 8 hi(P_16) + 1 <= 2^32 - 7
    for j in range(9):                                     # low limbs: signed chains
        for n, k in enumerate(subs):
            start = KBIAS if (j == 0 and n == 0) else D
            L.append(f"v_mad_i64_i32 {D}, {SD}, %{O[f's{n}'] + j}, -{k}, {start}")
        for (x, y) in terms_of_column(j):
            L.append(f"v_mad_u64_u32 {D}, {SD}, {opnd(x)}, {opnd(y)}, {D}")
        if j < 8:
            L.append(f"v_mad_u64_u32 {D}, {SD}, {lo(j + 9)}, {K31264}, {D}")
            if j:
                L.append(f"v_mad_u64_u32 {D}, {SD}, {lo(j + 8)}, {K256}, {D}")
            L.append(f"v_and_b32_e32 {r(j)}, 0x1fffffff, {d0}")
            L.append(f"v_ashrrev_i64 {D}, 29, {D}")
        else:
            L.append(f"v_mad_u64_u32 {D}, {SD}, {hi(16)}, {K250112}, {D}")  # 31264 o17
            L.append(f"v_mad_u64_u32 {D}, {SD}, {lo(16)}, {K256}, {D}")
            L.append(f"v_and_b32_e32 {r(8)}, 0xffffff, {d0}")
            L.append(f"v_ashrrev_i64 {D}, 24, {D}")
    T, t0, t1 = "v[6:7]", "v6", "v7"                      # P_10 is dead by now
    L.append(f"v_mad_u64_u32 {T}, {SD}, {c1}, {K8192}, {D}")  # T = (c >> 24) + (o17 + 1) 2^13 >= 0
    L.append(f"v_mov_b32 {d1}, 0")
    L.append(f"v_mov_b32 {d0}, {r(0)}")
    L.append(f"v_mad_u64_u32 {D}, {SD}, {t0}, {K977}, {D}")
    L.append(f"v_mad_u32_u24 {d1}, {t1}, {K977}, {d1}")
    L.append(f"v_and_b32_e32 {r(0)}, 0x1fffffff, {d0}")
    L.append(f"v_lshrrev_b64 {D}, 29, {D}")
    L.append(f"v_lshl_add_u64 {D}, {T}, 3, {D}")
    L.append(f"v_mad_u64_u32 {D}, {SD}, {r(1)}, 1, {D}")
    L.append(f"v_and_b32_e32 {r(1)}, 0x1fffffff, {d0}")
    L.append(f"v_alignbit_b32 {t0}, {d1}, {d0}, 29")
    L.append(f"v_add_u32 {r(2)}, {r(2)}, {t0}")
    return L


def full3s(name, doc, terms_of_column, subs):
    L = full_lines3s(terms_of_column, subs)
    sub_names = ["c", "d"][:len(subs)]
    outs = ", ".join([f'"=&v"(r[{i}])' for i in range(9)] + ['"=&s"(sd)'])
    ins = ", ".join([f'"v"(a[{i}])' for i in range(9)] + [f'"v"(b[{j}])' for j in range(9)] +
                    ['"s"(k31264)', '"s"(k256)', '"s"(k977)', '"s"(k8192)'] +
                    [f'"v"({s}[{j}])' for s in sub_names for j in range(9)] +
                    ['"s"(kbias)', '"s"(k250112)'])
    body = "\\n\\t".join(L)
    clob = ", ".join(f'"v{i}"' for i in range(2, 20))
    return [f"// {doc}",
            f"__device__ __forceinline__ void {name}(uint32_t r[9], const uint32_t a[9], const uint32_t b[9]"
            + "".join(f", const uint32_t {s}[9]" for s in sub_names) + ") {",
            "    uint64_t sd;",
            "    uint32_t k31264 = 31264u, k256 = 256u, k977 = 977u, k8192 = 8192u, k250112 = 250112u;",
            f"    int64_t kbias = {SUB_BIAS0}ll;  // -{SUB_K} (2^32 + 977)",
            f'    asm("{body}"',
            f"        : {outs}",
            f"        : {ins}",
            f"        : {clob});",
            "}"]


def full2(name, doc, terms_of_column, addend=False, dot=False, gen=None, third=False):
    """third: a third operand array c that the terms read (no addend, no d)"""
    L = (gen or full_lines2)(terms_of_column, addend)
    outs = ", ".join([f'"=&v"(r[{i}])' for i in range(9)] + ['"=&s"(sd)'])
    ins = ", ".join([f'"v"(a[{i}])' for i in range(9)] + [f'"v"(b[{j}])' for j in range(9)] +
                    ['"s"(k31264)', '"s"(k256)', '"s"(k977)', '"s"(k8192)'] +
                    ([f'"v"(c[{j}])' for j in range(9)] if addend or dot or third else []) +
                    ([f'"v"(d[{j}])' for j in range(9)] if dot else []))
    body = "\\n\\t".join(L)
    clob = ", ".join(f'"v{i}"' for i in range(2, 20))
    return [f"// {doc}",
            f"__device__ __forceinline__ void {name}(uint32_t r[9], const uint32_t a[9], const uint32_t b[9]"
            + (", const uint32_t c[9]" if addend or dot or third else "") + (", const uint32_t d[9]" if dot else "") + ") {",
            "    uint64_t sd;",
            "    uint32_t k31264 = 31264u, k256 = 256u, k977 = 977u, k8192 = 8192u;",
            f'    asm("{body}"',
            f"        : {outs}",
            f"        : {ins}",
            f"        : {clob});",
            "}"]

def main():
    out = ["// GENERATED by tools/gen_fe9_asm.py — do not edit by hand.",
           "// Column products of secp256k1_fe9.cuh as single inline-asm statements (see the generator's",
           "// docstring for why).  Column form 3: the low columns run inside the reduction's carry chain",
           "// (full_lines3).  Forms 1 (every column masked and shifted) and 2 (high columns 9..16 unmasked in",
           "// fixed register pairs) stay in the generator as the instruction emulator's references",
           "// (tests/test_asm_emulated.py); the kernels use form 3 only (r04: 175 -> 136 instructions a product).",
           "// The *_sub* statements are form 3 with subtrahends in signed low chains (full_lines3s).",
           "#pragma once", "#include <stdint.h>",
           "namespace gsv {"]
    specs = [("fe9_mul_full", "r = a * b mod p, weakly normalised (fe9_mul's contract)", MUL_TERMS, False, False),
             ("fe9_sqr_full", "r = a^2 mod p with b = 2a limb-wise (fe9_sqr's contract)", SQR_TERMS, False, False),
             ("fe9_mul_add_full", "r = a * b + c mod p, c limbs < 2^31 (fe9_mul_add's contract)", MUL_TERMS, True, False),
             ("fe9_sqr_add_full", "r = a^2 + c mod p with b = 2a limb-wise, c limbs < 2^31 (fe9_sqr_add's contract)",
              SQR_TERMS, True, False),
             ("fe9_dot_full", "r = a * b + c * d mod p, one reduction (fe9_dot's contract)", DOT_TERMS, False, True),
             ("fe9_dot_ms_full", "r = a * b + c^2 mod p with d = 2c limb-wise, one reduction (fe9_dot_ms's contract)",
              DOT_MS_TERMS, False, True),
             ("fe9_sqr3_full", "r = 3 a^2 mod p with b = 6a, c = 3a limb-wise (fe9_sqr3's contract)",
              SQR3_TERMS, False, "third")]
    for name, doc, terms, add, dot in specs:
        out += full2(name, doc, terms, add, dot is True, gen=full_lines3, third=dot == "third")
    sub_specs = [("fe9_mul_sub_full", "r = a * b - c mod p, c limbs < 2^31, m_a m_b <= 3.5 (fe9_mul_sub's contract)",
                  MUL_TERMS, [1]),
                 ("fe9_sqr_sub2_k1_full", "r = a^2 - c - d mod p with b = 2a limb-wise (fe9_sqr_sub2<1>'s contract)",
                  SQR_TERMS, [1, 1]),
                 ("fe9_sqr_sub2_k2_full", "r = a^2 - c - 2 d mod p with b = 2a limb-wise (fe9_sqr_sub2<2>'s contract)",
                  SQR_TERMS, [1, 2]),
                 ("fe9_sqr_sub1_k2_full", "r = a^2 - 2 c mod p with b = 2a limb-wise (fe9_sqr_sub2<2> without c)",
                  SQR_TERMS, [2])]
    for name, doc, terms, subs in sub_specs:
        out += full3s(name, doc, terms, subs)
    out.append("}  // namespace gsv")
    with open(OUT, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
