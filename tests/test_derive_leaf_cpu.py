"""CPU: tests/derive_leaf_model.py against oracle.derive_sha, and the tables of header and hashed lengths that
tests/test_gpu_derive_leaf.py relies on.  Nothing here reads the library."""
import random

import pytest

import derive_leaf_model as M

LENS = M.SWEEP_L + M.LONG_L


def _values(rng, L, n):
    """value sets of length L: for L = 1 one set of bytes below 0x80 (their own RLP) and one from 0x80 up"""
    if L == 1:
        return [[bytes([rng.randrange(0, 0x80)]) for _ in range(n)], [bytes([rng.randrange(0x80, 0x100)]) for _ in range(n)]]
    return [[rng.randbytes(L) for _ in range(n)]]


def test_one_item_list_is_its_leaf(oracle):
    rng = random.Random(1)
    assert M.depths(1) == [0] and M.compact(M.nibbles(0)) == b"\x20\x80"
    bad = []
    for L in LENS:
        for (v,) in _values(rng, L, 1):
            leaf = M.leaf_rlp(0, 0, v)
            if L != 1 or v[0] >= 0x80:
                assert len(leaf) == M.hashed_len("a", L), L
            if oracle.keccak256(leaf) != oracle.derive_sha([v]):
                bad.append((L, v[:1].hex()))
    assert not bad, bad


def _two_item_root(oracle, v0, v1):
    """the root of a two-item list: keys 0x80 and 0x01 part at the first nibble, so the root is a branch of 17
    slots with leaf 0 at nibble 8, leaf 1 at nibble 0 and no value"""
    assert M.nibbles(0) == [8, 0] and M.nibbles(1) == [0, 1] and M.depths(2) == [1, 1]
    slots = [b"\x80"] * 17
    for j, v in ((0, v0), (1, v1)):
        enc = M.leaf_rlp(j, 1, v)
        slots[M.nibbles(j)[0]] = b"\xa0" + oracle.keccak256(enc) if len(enc) >= 32 else enc
    return oracle.keccak256(oracle.rlp_list(b"".join(slots)))


def test_two_item_list_is_a_branch_of_two_leaves(oracle):
    rng = random.Random(2)
    bad = []
    for L in LENS:
        for v0, v1 in _values(rng, L, 2):
            if L != 1 or v0[0] >= 0x80:
                assert len(M.leaf_rlp(0, 1, v0)) == len(M.leaf_rlp(1, 1, v1)) == M.hashed_len("b", L), L
            if _two_item_root(oracle, v0, v1) != oracle.derive_sha([v0, v1]):
                bad.append((L, v0[:1].hex()))
    assert not bad, bad


# header bytes by value length: (H, first L, last L)
H_TABLE = {
    "a": [(5, 0, 51), (6, 52, 55), (7, 56, 250), (8, 251, 255), (9, 256, 65529), (10, 65530, 65535), (11, 65536, 70000)],
    "b": [(3, 0, 53), (4, 54, 55), (5, 56, 252), (6, 253, 255), (7, 256, 65531), (8, 65532, 65535), (9, 65536, 70000)],
}
UNREACHED = {"a": {57, 62, 258, 264, 65539, 65546}, "b": {57, 60, 258, 262, 65539, 65544}}


@pytest.mark.parametrize("cls", ["a", "b"])
def test_header_length_table(cls):
    got = [M.header_len(cls, L) for L in range(70001)]
    want = [0] * 70001
    for H, lo, hi in H_TABLE[cls]:
        want[lo:hi + 1] = [H] * (hi + 1 - lo)
    assert got == want
    assert max(H for H, _, _ in H_TABLE[cls]) <= 16  # the header fits k_derive_leaf's two registers


@pytest.mark.parametrize("cls", ["a", "b"])
def test_hashed_lengths_reached(cls):
    reached = {M.hashed_len(cls, L) for L in range(70001)}
    span = set(range(5, 432)) | set(range(65510, 65566))
    assert span - reached == UNREACHED[cls]
    swept = {M.hashed_len(cls, L) for L in M.SWEEP_L}
    assert set(M.BLOCK_TARGETS) & reached <= swept
    assert set(M.BLOCK_TARGETS) <= swept  # none of the unreached totals is a target
    edge = {M.hashed_len(cls, L) for L in M.EDGE_L}
    assert set(M.BLOCK_TARGETS) <= edge
    # the lengths the issue names
    first = "ab".index(cls) * 2
    assert [M.hashed_len(cls, L) for L in (26 + first, 27 + first, 28 + first)] == [31, 32, 33]
    assert [M.hashed_len(cls, L) for L in (129 + first, 263 + first, 399 + first)] == [136, 272, 408]
    long_reached = {M.hashed_len(cls, L) for L in M.LONG_L}
    assert set(range(65510, 65566)) & reached <= long_reached
    for H, lo, hi in H_TABLE[cls]:  # both sides of every change of H are swept
        if lo:
            assert {lo - 1, lo} <= set(M.EDGE_L) | set(M.LONG_L), lo


@pytest.mark.parametrize("N", [2, 17, 130, 300, 65836])
def test_leaves_below_a_branch_have_a_one_byte_key(N):
    d = M.depths(N)
    for j in range(N):
        ck = M.compact(M.nibbles(j)[d[j]:])
        assert len(ck) == 1 and ck[0] < 0x80, (N, j, ck.hex())
    assert M.CLASS_OF_N[N] == "b"


def test_three_item_list_is_class_b():
    # keys 80, 01, 02: leaf 0 one nibble below the root branch, leaves 1 and 2 below the branch that ends 0x0_
    assert M.depths(3) == [1, 2, 2]
    assert [M.compact(M.nibbles(j)[d:]).hex() for j, d in enumerate(M.depths(3))] == ["30", "20", "20"]
    assert M.CLASS_OF_N[3] == "b"
