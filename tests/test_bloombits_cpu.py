"""CPU tests of the bloombits family: the model (tests/bloombits_model.py) pinned to the data of the reference's own
tests (tests/golden/bloombits.json) and to two relations of them, the ABI pins of the new ids and codes, and the
entry points' argument checks, which come before any HIP call."""
import ctypes
import os
import random
import re

import numpy as np

import bloombits_model as M
from conftest import ROOT, golden

FX = golden("bloombits.json")


# ---------------------------------------------------------------- the codec
def test_encoding_cycle():
    assert len(FX["encoding_cycle"]) == 18
    for h in FX["encoding_cycle"]:
        data = bytes.fromhex(h)
        assert M.bitset_decode_bytes(M.bitset_encode_bytes(data), len(data)) == (data, M.ST_OK), h
        assert M.decompress_bytes(M.compress_bytes(data), len(data)) == (data, M.ST_OK), h


def test_decoding_cycle():
    seen = set()
    for row in FX["decoding_cycle"]:
        data = bytes.fromhex(row["input"])
        out, st = M.bitset_decode_bytes(data, row["size"])
        assert st == M.ERR_NAMES[row["fail"]], row
        seen.add(st)
        if st == M.ST_OK:
            assert M.bitset_encode_bytes(out) == data, row
    assert seen == {M.ST_OK, M.ST_MISSING_DATA, M.ST_UNREFERENCED_DATA, M.ST_EXCEEDED_TARGET, M.ST_ZERO_CONTENT}


def test_compression():
    for pair in FX["compression"]:
        a, b = bytes.fromhex(pair["in"]), bytes.fromhex(pair["out"])
        assert M.compress_bytes(a) == b
        assert M.decompress_bytes(b, len(a)) == (a, M.ST_OK)
    assert M.compress_bytes(bytes.fromhex("4912385c0e7b64000000")).hex() == "80fe4912385c0e7b64"
    long = FX["compression_long"]
    assert M.decompress_bytes(bytes.fromhex(long["input"]), long["size"]) == (None, M.ERR_NAMES[long["fail"]])
    # a dense vector's encoding is longer than the vector: 512 + 64 + 8 + 1
    assert len(M.bitset_encode_bytes(b"\x01" * 512)) == 585 and M.compress_bytes(b"\x01" * 512) == b"\x01" * 512
    assert M.compress_bytes(bytes(512)) == b"" and M.compress_bytes(b"") == b""


# ---------------------------------------------------------------- the generator
def test_generator_relation():
    """TestGenerator (generator_test.go:29-60): input i's bit j, MSB first, is output 2047 - j's bit i"""
    rng = random.Random(1)
    blooms = [bytes(rng.getrandbits(8) for _ in range(256)) for _ in range(2048)]
    g = M.Generator(2048)
    for i, b in enumerate(blooms):
        g.add_bloom(i, b)
    want = [bytearray(256) for _ in range(2048)]
    for i in range(2048):
        v = int.from_bytes(blooms[i], "big")
        for j in range(2048):
            if (v >> (2047 - j)) & 1:
                want[2047 - j][i // 8] |= 1 << (7 - i % 8)
    for i in range(2048):
        assert g.bitset(i) == bytes(want[i]), i
    arr = np.frombuffer(b"".join(blooms), np.uint8).reshape(2048, 256)
    assert M.generate_sections_np(arr, 2048).tobytes() == b"".join(bytes(w) for w in want)


def test_generator_errors_and_the_numpy_statement():
    for bad in (7, 12):
        try:
            M.Generator(bad)
            assert False
        except ValueError:
            pass
    g = M.Generator(8)
    for call in (lambda: g.add_bloom(1, bytes(256)), lambda: g.bitset(0)):
        try:
            call()
            assert False
        except ValueError:
            pass
    rng = random.Random(2)
    for s, n in ((8, 3), (72, 2), (16, 1)):
        blooms = [bytes(rng.getrandbits(8) & rng.getrandbits(8) for _ in range(256)) for _ in range(s * n)]
        arr = np.frombuffer(b"".join(blooms), np.uint8).reshape(-1, 256)
        assert M.generate_sections_np(arr, s).tobytes() == M.generate_sections(blooms, s)


# ---------------------------------------------------------------- the matcher
def test_new_matcher_drops_as_the_reference():
    w = FX["wildcards"]
    filters = [None if rule is None else [None if cl is None else bytes.fromhex(cl) for cl in rule]
               for rule in w["filters"]]
    assert [len(r) for r in M.kept_rules(filters)] == w["kept"] == [2, 2, 1]
    got = M.new_matcher_filters(filters)
    assert [len(r) for r in got] == [2, 2, 1] and all(len(cl) == 3 and max(cl) < 2048 for r in got for cl in r)
    assert M.kept_rules(None) == [] and M.kept_rules([[b""]]) == [[b""]]  # an empty clause that is not nil stays


def _cases():
    m = FX["matcher"]
    return m["section_size"], m["continuous"] + [m["shifted"]]


def test_match_agrees_with_exp_match3():
    """matcher_test.go: rows made as block % bit == 0, the expected set by expMatch3"""
    s, cases = _cases()
    assert s == 4096 and len(cases) == 3
    for case in cases:
        f, start, blocks = case["filter"], case["start"], case["blocks"]
        n_sections = (blocks - 1) // s + 1
        rows = {}

        def row(section, bit):
            if (section, bit) not in rows:
                rows[section, bit] = M.modulo_row(bit, section, s)
            return rows[section, bit]
        got = M.match_blocks(f, row, s, 0, n_sections, start, blocks - 1)
        assert got == [i for i in range(start, blocks) if M.exp_match3(f, i)], f
        assert got, f
        # the per-section bitsets and counts say the same
        total = sum(M.match_bitset(f, lambda b, k=k: row(k, b), s, k, start, blocks - 1)[1] for k in range(n_sections))
        assert total == len(got)
    # the wildcard: every block of the range (TestWildcardMatcher)
    assert M.match_blocks([], None, 8, 0, 2, 3, 12) == list(range(3, 13))


def test_bloom_filter_and_the_shared_rule_evaluation():
    rng = random.Random(5)
    items = [bytes(rng.getrandbits(8) for _ in range(n)) for n in (20, 20, 32, 32, 32, 32)]
    acc = 0
    for it in items[:4]:
        acc |= M.R.bloom9(it)
    bloom = M.R.to_bloom(acc)
    for addresses, topics in (([], []), (items[:1], []), (items[4:5], []), (items[:2], [items[2:3], []]),
                              ([], [[items[5]], [items[2]]]), ([], [[items[5], items[3]]]), (items[4:5] + items[1:2], [])):
        want = M.bloom_filter(bloom, addresses, topics)
        bits = M.new_matcher_filters(M.flatten(addresses, topics))
        assert M.filter_bits(bits, bloom) == want, (addresses, topics)


# ---------------------------------------------------------------- the ABI
def test_abi_pins_of_the_bloombits_family():
    from gsv import _lib
    txt = open(os.path.join(ROOT, "include", "gsv.h")).read()

    def val(name):
        return int(re.search(r"#define %s (\d+)" % name, txt).group(1))
    for k, name in enumerate(["MISSING_DATA", "UNREFERENCED_DATA", "EXCEEDED_TARGET", "ZERO_CONTENT"]):
        assert val("GSV_ST_BITSET_" + name) == getattr(_lib, "ST_BITSET_" + name) == getattr(M, "ST_" + name) == 37 + k
    assert [_lib.STATUS_STRINGS[37 + k] for k in range(4)] == ["missing bytes on input", "extra bytes on input",
                                                               "target data size exceeded", "zero byte in input content"]
    assert val("GSV_K_CREST") == _lib.K_CREST == 31  # pinned: the new ids are behind it
    for k, name in enumerate(["BLOOMBITS_GENERATE", "BITSET_COMPRESS", "BITSET_DECOMPRESS", "BLOOMBITS_MATCH",
                              "BLOOMBITS_TOTALS", "BLOOMBITS_SCAN", "BLOOMBITS_BLOCKS", "BLOOM_FILTER"]):
        assert val("GSV_K_" + name) == getattr(_lib, "K_" + name) == 31 + k
    assert val("GSV_K_RIDGE") == _lib.K_RIDGE == 39
    assert val("GSV_ABI_VERSION") == 2
    assert val("GSV_BLOOMBITS_MAX_SECTION") == _lib.BLOOMBITS_MAX_SECTION == 32768
    assert val("GSV_BITSET_MAX_LEN") == _lib.BITSET_MAX_LEN == 4096 and val("GSV_BLOOM_BITS") == _lib.BLOOM_BITS == 2048
    L = _lib.load()
    assert L.gsv_ctx_kernel_time(None, 38, None, None) == _lib.E_INVALID_ARG
    fake = ctypes.c_void_p(8)  # never dereferenced: the id check comes first
    assert L.gsv_ctx_kernel_time(fake, 39, None, None) == _lib.E_INVALID_ARG


def test_entry_points_check_their_arguments_without_a_device():
    from gsv import _lib
    L = _lib.load()
    E = _lib.E_INVALID_ARG
    fake = ctypes.c_void_p(8)  # a context that is never dereferenced
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 1)
    # NULL context, then NULL arrays
    assert L.gsv_bloombits_generate_batch(None, p, 1, 8, p) == E
    assert L.gsv_bloombits_generate_dev(None, p, 1, 8, p, None) == E
    assert L.gsv_bitset_compress_batch(None, p, 1, 8, p, p) == E
    assert L.gsv_bitset_compress_batch_dev(None, p, 1, 8, p, p, None) == E
    assert L.gsv_bitset_decompress_batch(None, p, p, 1, 8, p, p) == E
    assert L.gsv_bitset_decompress_batch_dev(None, p, p, 1, 8, p, p, None) == E
    assert L.gsv_bloombits_match_dev(None, p, 8, 0, 1, p, 1, p, 1, p, 1, p, p, p, p, None) == E
    assert L.gsv_bloombits_blocks_dev(None, p, p, 8, 0, 1, 1, p, p, 1, None) == E
    assert L.gsv_bloombits_match_batch(None, p, 8, 0, 1, p, p, p, p, p, 1, p, p, p, p, 1) == E
    assert L.gsv_bloom_filter_dev(None, p, 1, p, 1, p, 1, p, 1, p, None) == E
    assert L.gsv_bloom_filter_batch(None, p, 1, p, p, p, p, p, 1, p) == E
    assert L.gsv_bloombits_generate_batch(fake, None, 1, 8, p) == E and L.gsv_bloombits_generate_batch(fake, p, 1, 8, None) == E
    assert L.gsv_bloombits_generate_dev(fake, None, 1, 8, p, None) == E and L.gsv_bloombits_generate_dev(fake, p, 1, 8, None, None) == E
    # a bad S, everywhere one is taken
    for s in (0, 4, 7, 12, 32768 + 8, 65536):
        assert L.gsv_bloombits_generate_batch(fake, p, 1, s, p) == E, s
        assert L.gsv_bloombits_generate_dev(fake, p, 1, s, p, None) == E, s
        assert L.gsv_bloombits_match_dev(fake, p, s, 0, 1, p, 1, p, 1, p, 1, p, p, p, p, None) == E, s
        assert L.gsv_bloombits_blocks_dev(fake, p, p, s, 0, 1, 1, p, p, 1, None) == E, s
        assert L.gsv_bloombits_match_batch(fake, p, s, 0, 1, p, p, p, p, p, 1, p, p, p, p, 1) == E, s
    # nothing to do: success, nothing enqueued
    assert L.gsv_bloombits_generate_dev(fake, None, 0, 8, None, None) == 0
    assert L.gsv_bloombits_generate_batch(fake, None, 0, 32768, None) == 0
    assert L.gsv_bitset_compress_batch_dev(fake, None, 0, 1, None, None, None) == 0
    assert L.gsv_bitset_decompress_batch_dev(fake, None, None, 0, 4096, None, None, None) == 0
    assert L.gsv_bloombits_match_dev(fake, None, 8, 0, 3, None, 0, None, 0, None, 0, None, None, None, None, None) == 0
    assert L.gsv_bloombits_blocks_dev(fake, None, None, 8, 0, 3, 0, None, None, 0, None) == 0
    assert L.gsv_bloom_filter_dev(fake, None, 0, None, 0, None, 0, p, 1, None, None) == 0
    # the codec: a length of 0 or above 4,096, NULL arrays, a misaligned length array or table
    for bad in (0, 4097):
        assert L.gsv_bitset_compress_batch_dev(fake, p, 1, bad, p, p, None) == E
        assert L.gsv_bitset_decompress_batch_dev(fake, p, p, 1, bad, p, p, None) == E
        assert L.gsv_bitset_compress_batch(fake, p, 1, bad, p, p) == E
        assert L.gsv_bitset_decompress_batch(fake, p, p, 1, bad, p, p) == E
    assert L.gsv_bitset_compress_batch_dev(fake, p, 1, 8, p, odd, None) == E
    assert L.gsv_bitset_compress_batch_dev(fake, None, 1, 8, p, p, None) == E
    assert L.gsv_bitset_compress_batch_dev(fake, p, 1, 8, None, p, None) == E
    assert L.gsv_bitset_compress_batch_dev(fake, p, 1 << 31, 8, p, p, None) == E
    assert L.gsv_bitset_decompress_batch_dev(fake, p, odd, 1, 8, p, p, None) == E
    assert L.gsv_bitset_decompress_batch_dev(fake, p, None, 1, 8, p, p, None) == E
    assert L.gsv_bitset_decompress_batch_dev(fake, p, p, 1, 8, None, p, None) == E
    assert L.gsv_bitset_decompress_batch_dev(fake, p, p, 1, 8, p, None, None) == E
    back = (ctypes.c_uint64 * 2)(5, 3)
    assert L.gsv_bitset_decompress_batch(fake, p, ctypes.cast(back, ctypes.c_void_p), 1, 8, p, p) == E
    # the matcher: each required array, each alignment, the bounds on sections, queries and pairs
    ok = [fake, p, 8, 0, 1, p, 1, p, 1, p, 1, p, p, p, p, None]

    def match_dev(**k):
        a = list(ok)
        for i, v in k.items():
            a[int(i[1:])] = v
        return L.gsv_bloombits_match_dev(*a)
    for k in (dict(_1=None), dict(_5=None), dict(_5=odd), dict(_7=None), dict(_7=odd), dict(_9=None), dict(_9=odd),
              dict(_11=None), dict(_11=odd), dict(_12=None), dict(_12=odd), dict(_13=None), dict(_14=None),
              dict(_14=odd), dict(_4=(1 << 20) + 1), dict(_10=(1 << 20) + 1), dict(_4=1 << 13, _10=(1 << 11) + 1),
              dict(_6=(1 << 20) + 1), dict(_8=(1 << 20) + 1), dict(_3=(1 << 40) + 1)):
        assert match_dev(**k) == E, k
    assert L.gsv_bloombits_blocks_dev(fake, p, p, 8, 0, 1, 1, None, p, 1, None) == E
    assert L.gsv_bloombits_blocks_dev(fake, p, p, 8, 0, 1, 1, odd, p, 1, None) == E
    assert L.gsv_bloombits_blocks_dev(fake, p, p, 8, 0, 1, 1, p, None, 1, None) == E
    assert L.gsv_bloombits_blocks_dev(fake, p, p, 8, 0, 1, 1, p, odd, 1, None) == E
    assert L.gsv_bloombits_blocks_dev(fake, None, p, 8, 0, 1, 1, p, p, 1, None) == E
    assert L.gsv_bloombits_blocks_dev(fake, p, odd, 8, 0, 1, 1, p, p, 1, None) == E
    # the host forms: a missing table, a table that steps backwards
    one = (ctypes.c_uint64 * 2)(0, 1)
    po = ctypes.cast(one, ctypes.c_void_p)
    pb = ctypes.cast(back, ctypes.c_void_p)
    assert L.gsv_bloombits_match_batch(fake, p, 8, 0, 1, p, po, None, po, None, 1, p, p, p, p, 1) == E
    assert L.gsv_bloombits_match_batch(fake, p, 8, 0, 1, p, po, None, po, pb, 1, p, p, p, p, 1) == E
    assert L.gsv_bloombits_match_batch(fake, p, 8, 0, 1, p, po, None, None, po, 1, p, p, p, p, 1) == E
    assert L.gsv_bloombits_match_batch(fake, p, 8, 0, 1, p, po, None, po, po, 1, None, p, p, p, 1) == E
    assert L.gsv_bloombits_match_batch(fake, None, 8, 0, 1, p, po, None, po, po, 1, p, p, p, p, 1) == E
    assert L.gsv_bloom_filter_batch(fake, None, 1, p, po, None, po, po, 1, p) == E
    assert L.gsv_bloom_filter_batch(fake, p, 1, p, po, None, po, pb, 1, p) == E
    assert L.gsv_bloom_filter_batch(fake, p, 1, p, po, None, po, po, 1, None) == E
    assert L.gsv_bloom_filter_dev(fake, None, 1, p, 1, p, 1, p, 1, p, None) == E
    assert L.gsv_bloom_filter_dev(fake, p, 1, odd, 1, p, 1, p, 1, p, None) == E
    assert L.gsv_bloom_filter_dev(fake, p, 1, p, 1, p, 1, p, 1, None, None) == E
    assert L.gsv_bloom_filter_dev(fake, p, 1 << 17, p, 1, p, 1, p, 1 << 16, p, None) == E  # 2^33 verdicts


def test_python_wrappers_answer_without_a_launch():
    """target == 0, an empty vector, a bad section count: the wrappers decide before any library call"""
    import pytest
    from gsv import bitutil, bloombits
    assert bitutil.DecompressBytes(b"", 0) == b""
    with pytest.raises(bitutil.ErrExceededTarget, match="target data size exceeded"):
        bitutil.DecompressBytes(b"\x01", 0)
    assert bitutil.CompressBytes(b"") == b""
    with pytest.raises(ValueError):
        bitutil.CompressBytes(bytes(4097))
    with pytest.raises(bloombits.ErrSectionCount, match="section count not multiple of 8"):
        bloombits.NewGenerator(12)
    with pytest.raises(ValueError):
        bloombits.NewGenerator(32776)
    g = bloombits.NewGenerator(8)
    with pytest.raises(bloombits.ErrUnexpectedIndex):
        g.AddBloom(1, bytes(256))
    with pytest.raises(bloombits.ErrNotGenerated):
        g.Bitset(0)
    for k in range(8):
        g.AddBloom(k, bytes(256))
    with pytest.raises(bloombits.ErrSectionOutOfBounds):
        g.AddBloom(8, bytes(256))
    with pytest.raises(bloombits.ErrSectionOutOfBounds):
        g.Bitset(8)
    from gsv import filters
    f = filters.Filter([b"\x01" * 20], [[b"\x02" * 32, b"\x03" * 32], []])
    assert f.filters == [[b"\x01" * 20], [b"\x02" * 32, b"\x03" * 32], []]
    assert filters.Filter([], []).filters == []
