"""CPU checks of the collation-header corpus (tests/header_cases.py) that tests/test_gpu_header.py runs
on the GPU: the corpus reaches the lengths, list-header forms and statuses it is there for, and the
oracle's collation_header_rlp decodes back to each case's five fields under an RLP decoder written here
(so the expected hashes do not rest on the oracle's encoder agreeing with itself)."""
from collections import Counter

import pytest

import header_cases as H


@pytest.fixture(scope="module")
def cases(oracle):
    return H.corpus(oracle)


def test_length_matrix_reaches_every_rlp_length(cases):
    a = [c for c in cases if c.family == "a"]
    assert len(a) == 33 * 33 * 4 and all(c.sig65 is not None for c in a)
    signed = Counter(len(c.rlp) for c in a)
    assert set(signed) == set(range(73, 190))
    # the one-block / two-block boundary of Keccak-256's 136-byte rate and the pad byte either side
    assert signed[135] == signed[136] == signed[137] == 68
    unsigned = {len(c.unsigned_rlp) for c in a}
    assert min(unsigned) == 6 and max(unsigned) == 123
    # 0xc0 + n up to a payload of 55, 0xf8 n from 56: 57 bytes in all cannot occur
    assert unsigned == set(range(6, 124)) - {57}
    assert {c.unsigned_rlp[0] for c in a if len(c.unsigned_rlp) == 56} == {0xc0 + 55}
    assert {c.unsigned_rlp[:2] for c in a if len(c.unsigned_rlp) == 58} == {b"\xf8\x38"}
    assert all(c.rlp[0] == 0xf8 and c.rlp[1] == len(c.rlp) - 2 for c in a)


def test_families_and_statuses(cases):
    n = Counter(c.family for c in cases)
    assert n["a"] == 4356 and n["b"] == 16 and n["c"] == 1024 and n["d"] == 24
    assert {c.status for c in cases} == H.ALL_STATUSES
    for c in cases:
        assert (c.status == H.ST_INVALID_SIG_LEN) == bool(c.nil & 4), c.label
        assert any(c.signer) == (c.status in (H.ST_OK, H.ST_PROPOSER_MISMATCH)), c.label
    assert all(c.status == H.ST_OK for c in cases if c.family in "ab" and not c.nil & 2)
    assert all(c.status == H.ST_PROPOSER_MISMATCH for c in cases if c.family in "ab" and c.nil & 2)
    rnd = [c for c in cases if c.family == "c"]
    assert {c.nil for c in rnd} == set(range(8))
    assert sum(len(c.rlp) == 189 and c.nil == 0 for c in rnd) >= 250  # a first byte of zero shortens a few
    d = {c.label: c for c in cases if c.family == "d"}
    for nil0 in (0, 1):
        assert d[f"d: high-s twin, recid flipped, nil {nil0}"].status == H.ST_OK
        assert d[f"d: nil proposer, valid signature, nil {nil0 | 2}"].status == H.ST_PROPOSER_MISMATCH
        assert d[f"d: proposer differs in byte 0, nil {nil0}"].status == H.ST_PROPOSER_MISMATCH
        assert d[f"d: proposer differs in byte 19, nil {nil0}"].status == H.ST_PROPOSER_MISMATCH
        assert d[f"d: recid 4, nil {nil0}"].status == d[f"d: recid 255, nil {nil0}"].status == H.ST_INVALID_RECID
        assert d[f"d: r is no x-coordinate, nil {nil0}"].status == H.ST_RECOVER_FAILED
        assert d[f"d: nil signature over a valid signature, nil {nil0 | 4}"].sig_row != bytes([H.FILL]) * 65


def test_rows_fill_nil_fields_with_a5(cases):
    fill = bytes([H.FILL])
    for c in cases:
        sid, root, per, prop, sig = c.rows()
        assert [len(x) for x in (sid, root, per, prop, sig)] == [32, 32, 32, 20, 65]
        assert (root == fill * 32) == bool(c.nil & 1) and (prop == fill * 20) == bool(c.nil & 2), c.label
        if c.nil & 4 and "over" not in c.label:
            assert sig == fill * 65, c.label
    arrays = H.pack(cases[:300])
    assert [a.shape for a in arrays] == [(300, 32), (300, 32), (300, 32), (300, 20), (300, 65), (300,)]
    assert bytes(arrays[4][7]) == cases[7].sig65 and arrays[5][299] == cases[299].nil


def _item(b, pos):
    """one RLP item at b[pos:] -> (is_list, payload, next position); canonical forms only
    (rlp/decode.go: ErrCanonSize for a single byte below 0x80 in a string, for a long form under 56
    bytes and for a length with a leading zero)"""
    t = b[pos]
    if t < 0x80:
        return False, b[pos:pos + 1], pos + 1
    base = 0x80 if t < 0xc0 else 0xc0
    if t - base < 56:
        n, start = t - base, pos + 1
        assert base == 0xc0 or n != 1 or b[start] >= 0x80, "single byte below 0x80 with a prefix"
    else:
        ll = t - base - 55
        assert b[pos + 1] != 0, "length with a leading zero"
        n, start = int.from_bytes(b[pos + 1:pos + 1 + ll], "big"), pos + 1 + ll
        assert n >= 56, "long form under 56 bytes"
    assert start + n <= len(b), "item past the end"
    return base == 0xc0, b[start:start + n], start + n


def _fields(rlp):
    is_list, payload, end = _item(rlp, 0)
    assert is_list and end == len(rlp)
    out, pos = [], 0
    while pos < len(payload):
        sub_list, item, pos = _item(payload, pos)
        assert not sub_list
        out.append(item)
    return out


def _integer(item):
    assert not item or item[0] != 0, "integer with a leading zero"
    return int.from_bytes(item, "big")


def test_oracle_rlp_decodes_back_to_the_fields(cases):
    assert _fields(bytes.fromhex("c50180018080")) == [b"\x01", b"", b"\x01", b"", b""]
    for c in cases:
        for rlp, sig in ((c.rlp, c.sig65 or b""), (c.unsigned_rlp, b"")):
            f = _fields(rlp)
            assert len(f) == 5, c.label
            assert _integer(f[0]) == c.shard_id and _integer(f[2]) == c.period, c.label
            assert f[1] == (c.chunk_root or b"") and f[3] == (c.proposer or b"") and f[4] == sig, c.label
