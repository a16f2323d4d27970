"""TEST INFRASTRUCTURE — a restatement of the leaves of types.DeriveSha's trie (core/types/derive_sha.go:32-41,
trie/hasher.go:113-145, trie/encoding.go hexToCompact) over oracle.rlp_uint / rlp_string / rlp_list, and the
value lengths that tests/test_gpu_derive_leaf.py sweeps.  It never reads the library: tests/test_derive_leaf_cpu.py
pins it to oracle.derive_sha.

Item j's key is rlp(uint(j)).  Its leaf sits 1 + (the longest prefix, in nibbles, that its key shares with
another key of the list) nibbles deep: the branch below the shared prefix takes one nibble more.  A list of
one item is that leaf at depth 0.  The leaf is [compact(key nibbles past the depth), value]; k_derive_leaf
hashes header || value, T = H + L bytes, where H covers the list prefix, the key and the value's prefix."""
from __future__ import annotations

from oracle import oracle as O

RATE = 136  # Keccak-256 rate in bytes


def nibbles(j: int) -> list[int]:
    """the key of item j, rlp(uint(j)), in nibbles (trie/encoding.go keybytesToHex without the terminator)"""
    return [n for b in O.rlp_uint(j) for n in (b >> 4, b & 15)]


def _lcp(a, b) -> int:
    n = 0
    while n < min(len(a), len(b)) and a[n] == b[n]:
        n += 1
    return n


def depths(N: int) -> list[int]:
    """depth of leaf j in a list of N items, for every j"""
    if N == 1:
        return [0]
    order = sorted(range(N), key=nibbles)  # the longest shared prefix is with a neighbour in key order
    keys = [nibbles(j) for j in order]
    out = [0] * N
    for p, j in enumerate(order):
        near = [keys[q] for q in (p - 1, p + 1) if 0 <= q < N]
        out[j] = 1 + max(_lcp(keys[p], k) for k in near)
    return out


def compact(rem: list[int]) -> bytes:
    """hexToCompact of a leaf's remaining nibbles (terminator flag 2, odd flag 1)"""
    if len(rem) % 2:
        head, rest = bytes([0x30 | rem[0]]), rem[1:]
    else:
        head, rest = b"\x20", rem
    return head + bytes(rest[k] << 4 | rest[k + 1] for k in range(0, len(rest), 2))


def leaf_rlp(j: int, depth: int, value: bytes) -> bytes:
    return O.rlp_list(O.rlp_string(compact(nibbles(j)[depth:])) + O.rlp_string(value))


# the two leaf classes: the encoded compact key of a one-item list (82 20 80) and of a leaf below a branch
# whose compact key is one byte below 0x80 (itself)
KEY_ENC = {"a": 3, "b": 1}
CLASS_OF_N = {1: "a", 2: "b", 3: "b", 17: "b", 130: "b", 300: "b", 65836: "b"}


def _prefix(n: int) -> int:
    """bytes of the RLP string or list prefix of an n-byte payload (rlp/encode.go:71-89)"""
    return 1 if n < 56 else 1 + (n.bit_length() + 7) // 8


def hashed_len(cls: str, L: int) -> int:
    """T: bytes of the leaf's RLP for a value of L bytes that is not a single byte below 0x80"""
    payload = KEY_ENC[cls] + _prefix(L) + L
    return _prefix(payload) + payload


def header_len(cls: str, L: int) -> int:
    return hashed_len(cls, L) - L


# ---- the lengths the GPU tests use
SWEEP_L = tuple(range(0, 421))          # T up to 3 * 136 + 21: three rate-block edges, every short-prefix H
LONG_L = tuple(range(65500, 65560))     # the two- to three-byte length prefixes of the string and of the list
BLOCK_TARGETS = tuple(sorted({31, 32, 33} | {RATE * k + d for k in (1, 2, 3) for d in range(-2, 3)}))


def edge_l(cls: str, lens=SWEEP_L) -> list[int]:
    """every L whose T is within 2 of the inline threshold (32) or of a multiple of the rate (136, 272, 408),
    and both sides of every change of H"""
    out = set()
    for L in lens:
        T = hashed_len(cls, L)
        if any(abs(T - e) <= 2 for e in (32, RATE, 2 * RATE, 3 * RATE)):
            out.add(L)
        if L + 1 in lens and header_len(cls, L) != header_len(cls, L + 1):
            out |= {L, L + 1}
    return sorted(out)


EDGE_L = tuple(sorted(set(edge_l("a")) | set(edge_l("b"))))
