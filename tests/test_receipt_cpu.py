"""CPU tests of the receipt path's model (tests/receipt_model.py), pinned to the reference: TestBloom's words
(core/types/bloom9_test.go:24-51), the bit layout the bloombits generator states (core/bloombits/generator.go:64-70),
EmptyRootHash, decode-then-encode, and every expected status of the shared corpus (tests/receipt_cases.py).  Then
the ABI: the new constants in include/gsv.h equal the binding's, and every new entry point returns its argument
errors without a GPU."""
import json
import os
import re

import receipt_cases as C
import receipt_model as R
from conftest import GOLDEN, ROOT


# ---------------------------------------------------------------- bloom9
def test_bloom_test_words():
    """TestBloom (bloom9_test.go:24-51): four words in, two words that must test false"""
    want = {b"testtest": [1303, 70, 1533], b"test": [1058, 1887, 496], b"hallo": [291, 168, 806],
            b"other": [1718, 875, 1586]}
    acc = 0
    for w, idx in want.items():
        assert R.bloom_indexes(w) == idx, w
        acc |= R.bloom9(w)
    bloom = R.to_bloom(acc)
    for w in want:
        assert R.bloom_lookup(bloom, w)
    for w in (b"tes", b"lo"):
        assert not R.bloom_lookup(bloom, w)
    assert R.bloom_indexes(bytes(20)) == [896, 1975, 1665] and R.bloom_indexes(bytes(32)) == [269, 1241, 1163]


def test_bit_layout_is_the_generators():
    """generator.go:64-70: bit i of a Bloom is bloom[BloomByteLength - 1 - i / 8] under mask byte(1) << (i % 8)"""
    for b in (0, 1, 7, 8, 1303, 2040, 2047):
        row = R.to_bloom(1 << b)
        assert row[R.BLOOM_BYTES - 1 - b // 8] == 1 << (b % 8) and sum(row) == 1 << (b % 8)
    r = R.new_receipt(logs=[(bytes(20), [bytes(32)], b"")])
    bits = sorted([896, 1975, 1665, 269, 1241, 1163])
    assert [k for k in range(2048) if int.from_bytes(r["bloom"], "big") >> k & 1] == bits
    assert R.create_bloom([r, r]) == r["bloom"] == R.logs_bloom(r["logs"])


def test_empty_list():
    st, bloom, root, gas, sts = R.validate([])
    assert (st, bloom, gas, sts) == (R.ST_OK, bytes(256), 0, [])
    assert root == R.EMPTY_ROOT == R.keccak256(b"\x80")  # types.EmptyRootHash


# ---------------------------------------------------------------- decode
def test_corpus_statuses_and_round_trip():
    corpus = C.decode_corpus()
    seen = set()
    for name, blob, want in corpus:
        st, r = R.decode_status(blob)
        assert st == want, name
        seen.add(st)
        if r is not None:
            assert R.encode_receipt(r) == blob, name  # canonical encodings only: decode then encode is the identity
    assert seen == {R.ST_OK, R.ST_BAD_RLP, R.ST_RECEIPT_STATUS}
    names = [n for n, _, _ in corpus]
    assert len(set(names)) == len(names) > 80
    sizes = {len(b) for _, b, _ in corpus}
    assert max(sizes) > 65536 and 0 in sizes
    for target in (55, 56, 255, 256):
        r = R.decode_receipt(C.with_logs_payload(target))
        assert len(b"".join(R.encode_log(g) for g in r["logs"])) == target
    # seven topics decode: the decoder has no cap of four
    assert len(R.decode_receipt(dict((n, b) for n, b, _ in corpus)["7 topics"])["logs"][0][1]) == 7


def test_random_receipts_round_trip():
    for lst in C.random_lists(5, [40]):
        for blob in lst:
            assert R.encode_receipt(R.decode_receipt(blob)) == blob


def test_validate_order():
    lst = C.random_lists(9, [5])[0]
    st, bloom, root, gas, _ = R.validate(lst)
    assert st == R.ST_OK and gas == R.decode_receipt(lst[-1])["gas"] and root == R.derive_sha(lst)
    other = bytes(x ^ 1 for x in bloom)
    assert R.validate(lst, bloom, root, gas)[0] == R.ST_OK
    assert R.validate(lst, other, bytes(32), gas + 1)[0] == R.ST_GAS_USED_MISMATCH
    assert R.validate(lst, other, bytes(32), gas)[0] == R.ST_INVALID_BLOOM
    assert R.validate(lst, other, bytes(32), None)[0] == R.ST_INVALID_BLOOM
    assert R.validate(lst, bloom, bytes(32), gas)[0] == R.ST_INVALID_RECEIPT_ROOT
    assert R.validate(lst, None, None, None)[0] == R.ST_OK
    bad = lst[:2] + [C.raw(status=b"\x02")] + [b"\xc0"] + lst[2:]
    assert R.validate(bad, other, bytes(32), gas + 1)[:4] == (R.ST_RECEIPT_STATUS, bytes(256), bytes(32), 0)


def test_fixture_is_what_the_model_gives():
    with open(os.path.join(GOLDEN, "receipts.json")) as f:
        fx = json.load(f)
    assert 24 <= len(fx["lists"]) <= 64
    for e in fx["lists"]:
        blobs = [bytes.fromhex(x) for x in e["receipts"]]
        st, bloom, root, gas, sts = R.validate(blobs)
        assert (st, bloom.hex(), root.hex(), gas, sts) == (e["status"], e["bloom"], e["root"], e["gas_used"],
                                                            e["receipt_status"]), e["name"]
    assert {e["status"] for e in fx["lists"]} == {R.ST_OK, R.ST_BAD_RLP, R.ST_RECEIPT_STATUS}
    for w in fx["bloom9"]:
        assert R.bloom_indexes(bytes.fromhex(w["data"])) == w["indexes"]


# ---------------------------------------------------------------- the ABI
def test_abi_pins_of_the_receipt_path():
    from gsv import _lib
    txt = open(os.path.join(ROOT, "include", "gsv.h")).read()

    def val(name):
        return int(re.search(r"#define %s (\d+)" % name, txt).group(1))
    for k, name in enumerate(["RECEIPT_STATUS", "GAS_USED_MISMATCH", "INVALID_BLOOM", "INVALID_RECEIPT_ROOT"]):
        assert val("GSV_ST_" + name) == getattr(_lib, "ST_" + name) == getattr(R, "ST_" + name) == 33 + k
        assert getattr(_lib, "ST_" + name) in _lib.STATUS_STRINGS
    assert val("GSV_ST_BAD_RLP") == R.ST_BAD_RLP == _lib.ST_BAD_RLP
    assert val("GSV_K_SUMMIT") == _lib.K_SUMMIT == 26  # pinned: the new ids are behind it
    for k, name in enumerate(["RECEIPT_SCAN", "RECEIPT_BLOOM", "RECEIPT_LISTS", "RECEIPT_CHECK", "BLOOM9"]):
        assert val("GSV_K_" + name) == getattr(_lib, "K_" + name) == 26 + k
    assert val("GSV_K_CREST") == _lib.K_CREST == 31
    assert val("GSV_ABI_VERSION") == 2


def test_entry_points_check_their_arguments_without_a_device():
    import ctypes

    from gsv import _lib
    L = _lib.load()
    E = _lib.E_INVALID_ARG
    # the work area: 8 bytes per slot of 21 bytes of RLP, 12 per receipt, padded to 8; 0 past the bounds
    assert L.gsv_receipts_work_bytes(0, 0) == 8 and L.gsv_receipts_work_bytes(1, 20) == 8 + 16
    assert L.gsv_receipts_work_bytes(3, 21) == 16 + 24 + 16 and L.gsv_receipts_work_bytes(2, 2100) == 101 * 8 + 24
    assert L.gsv_receipts_work_bytes(1 << 31, 0) == 0 and L.gsv_receipts_work_bytes(1, (1 << 40) + 1) == 0
    assert L.gsv_receipts_work_bytes(1, 1 << 40) > (1 << 40) // 21 * 8
    assert L.gsv_bloom9_batch(None, None, None, 1, None) == E
    assert L.gsv_bloom9_batch_dev(None, None, None, 1, None, None) == E
    assert L.gsv_receipts_bloom_dev(None, None, None, 1, None, 1, 0, None, None, None, None, None, None, None) == E
    assert L.gsv_receipts_check_dev(None, None, None, None, None, None, None, None, 1, None, None) == E
    assert L.gsv_receipts_verify_batch(None, None, None, None, 1, None, None, None, None, None, None, None, None) == E
    # a context that is never dereferenced: the argument checks come before any HIP call
    fake = ctypes.c_void_p(8)
    one = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(one, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 1)
    assert L.gsv_bloom9_batch(fake, None, None, 1, None) == E
    assert L.gsv_bloom9_batch(fake, None, None, 0, None) == 0  # n == 0: success, nothing launched
    assert L.gsv_bloom9_batch_dev(fake, p, p, 1 << 32, p, None) == E
    assert L.gsv_bloom9_batch_dev(fake, p, odd, 1, p, None) == E and L.gsv_bloom9_batch_dev(fake, p, p, 1, odd, None) == E
    assert L.gsv_bloom9_batch_dev(fake, None, None, 0, None, None) == 0
    ok = [fake, p, p, 1, p, 1, 64, p, p, None, p, p, p, None]

    def bloom_dev(**k):
        a = list(ok)
        for i, v in k.items():
            a[int(i[1:])] = v
        return L.gsv_receipts_bloom_dev(*a)
    assert bloom_dev(_5=0) == 0  # no lists: success, nothing enqueued
    for k in (dict(_2=odd), dict(_4=odd), dict(_7=odd), dict(_11=odd), dict(_1=None), dict(_2=None), dict(_4=None),
              dict(_7=None), dict(_8=None), dict(_10=None), dict(_11=None), dict(_12=None), dict(_3=1 << 31),
              dict(_5=1 << 31), dict(_6=(1 << 40) + 1)):
        assert bloom_dev(**k) == E, k
    assert L.gsv_receipts_check_dev(fake, None, None, None, None, None, None, None, 0, None, None) == 0
    assert L.gsv_receipts_check_dev(fake, p, p, p, odd, None, None, None, 1, p, None) == E
    assert L.gsv_receipts_check_dev(fake, p, p, p, p, None, None, odd, 1, p, None) == E
    assert L.gsv_receipts_check_dev(fake, p, p, None, p, None, None, None, 1, p, None) == E
    assert L.gsv_receipts_check_dev(fake, p, p, p, p, None, None, None, 1, None, None) == E
    assert L.gsv_receipts_verify_batch(fake, None, None, None, 0, None, None, None, None, None, None, None, None) == 0
    off = (ctypes.c_uint64 * 3)(0, 5, 3)
    po = ctypes.cast(off, ctypes.c_void_p)
    lo = (ctypes.c_uint64 * 2)(0, 2)
    pl = ctypes.cast(lo, ctypes.c_void_p)
    assert L.gsv_receipts_verify_batch(fake, p, po, pl, 1, None, None, None, None, None, None, None, None) == E  # status
    assert L.gsv_receipts_verify_batch(fake, p, po, pl, 1, None, None, None, None, None, None, None, p) == E  # backwards
    back = (ctypes.c_uint64 * 2)(2, 0)
    assert L.gsv_receipts_verify_batch(fake, p, po, ctypes.cast(back, ctypes.c_void_p), 1, None, None, None, None, None,
                                       None, None, p) == E
    big = (ctypes.c_uint64 * 2)(0, 1 << 32)
    one_list = (ctypes.c_uint64 * 2)(0, 1)
    assert L.gsv_receipts_verify_batch(fake, p, ctypes.cast(big, ctypes.c_void_p), ctypes.cast(one_list, ctypes.c_void_p),
                                       1, None, None, None, None, None, None, None, p) == _lib.E_TOO_LARGE
