"""CPU tests of the ethash family: the numpy model (tests/ethash_model.py) against the recorded results of
the reference's libethash (tests/golden/ethash.json), the host code (csrc/ethash_host.h, csrc/ethash_mod.h)
as a stand-alone program under sanitizers, the model at a real row count, and the ABI's pinned values."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ethash_model as M
from conftest import ROOT, golden


@pytest.fixture(scope="module")
def fx():
    return golden("ethash.json")


def _rows(rows):
    h = np.frombuffer(bytes.fromhex("".join(r["hash"] for r in rows)), np.uint8).reshape(-1, 32)
    n = np.array([r["nonce"] for r in rows], np.uint64)
    mix = np.frombuffer(bytes.fromhex("".join(r["mix"] for r in rows)), np.uint8).reshape(-1, 32)
    res = np.frombuffer(bytes.fromhex("".join(r["result"] for r in rows)), np.uint8).reshape(-1, 32)
    return h, n, mix, res


# ---------------------------------------------------------------- the model against the fixture
def test_model_small_caches(fx):
    """generateCache at 1,024 bytes: TestCacheGeneration's epochs 0 and 1"""
    t = fx["test_mode"]
    seed1 = bytes.fromhex(next(s["seed"] for s in fx["sizes"] if s["block"] == 30000))
    assert M.generate_cache(1024, bytes(32)).tobytes().hex() == t["cache0"]
    assert M.generate_cache(1024, seed1).tobytes().hex() == t["cache1"]


@pytest.fixture(scope="module")
def small(fx):
    cache = M.words(bytes.fromhex(fx["test_mode"]["cache0"]))
    dataset = M.dataset_item(cache, np.arange(512, dtype=np.uint32))
    return cache, dataset


def test_model_small_dataset(fx, small):
    """generateDataset at 32 KiB: TestDatasetGeneration"""
    _, dataset = small
    assert M.keccak256_bytes(M.item_bytes(dataset)).hex() == fx["test_mode"]["dataset_digest"]


def test_model_go_vector_light_and_full(fx, small):
    """TestHashimoto (algorithm_test.go:657-686): light and full give the recorded digest and result"""
    cache, dataset = small
    go = fx["test_mode"]["go"]
    h = np.frombuffer(bytes.fromhex(go["hash"]), np.uint8).reshape(1, 32)
    for d, r in (M.hashimoto_light(32 * 1024, cache, h, [go["nonce"]]),
                 M.hashimoto_full(32 * 1024, dataset, h, [go["nonce"]])):
        assert d[0].tobytes().hex() == go["digest"] and r[0].tobytes().hex() == go["result"]


def test_model_test_mode_rows(fx, small):
    cache, dataset = small
    h, n, mix, res = _rows(fx["test_mode"]["light"])
    assert len(n) == 32
    d, r = M.hashimoto_light(32 * 1024, cache, h, n)
    assert (d == mix).all() and (r == res).all()
    d, r = M.hashimoto_full(32 * 1024, dataset, h, n)
    assert (d == mix).all() and (r == res).all()


# ---------------------------------------------------------------- the host code, as a program under sanitizers
def test_host_code_as_a_program_under_sanitizers(tmp_path, fx):
    """csrc/ethash_host.h and csrc/ethash_mod.h through tests/native/ethash_host_main.cpp with ASan + UBSan (a
    plain build where the compiler links neither), run as a child process: sizes and seeds of every fixture
    row, the two 2,048-entry digests, both 1 KiB caches, the full epoch-0 cache's digest and sampled rows
    (hence -O2), and the reciprocal reduction against %."""
    data = tmp_path / "ethash_rows.txt"
    with open(data, "w") as f:
        for s in fx["sizes"]:
            f.write(f"size {s['block']} {s['cache_size']} {s['dataset_size']} {s['seed']}\n")
        f.write(f"sizes_digest {fx['cache_sizes_digest']} {fx['dataset_sizes_digest']}\n")
        f.write(f"small_cache 0 1024 {fx['test_mode']['cache0']}\n")
        f.write(f"small_cache 30000 1024 {fx['test_mode']['cache1']}\n")
        f.write(f"full_cache 0 {fx['caches']['0']['digest']}\n")
        for r in fx["caches"]["0"]["rows"]:
            f.write(f"full_row {r['row']} {r['bytes']}\n")
    src = os.path.join(ROOT, "tests", "native", "ethash_host_main.cpp")
    exe = tmp_path / "ethash_host_main"
    base = ["g++", "-O2", "-g", "-std=c++17", "-Wall", "-o", str(exe), src]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ---------------------------------------------------------------- the model at a real row count
@pytest.fixture(scope="module")
def cache0():
    """the epoch-0 cache made by the library's host code (the plain build), read back through ctypes"""
    from gsv import ethash as E
    return E.generateCache(E.cacheSize(0), E.seedHash(0))


def test_library_cache_epoch0(fx, cache0):
    c = fx["caches"]["0"]
    assert len(cache0) == 16776896
    for r in c["rows"]:
        assert cache0[r["row"] * 64:(r["row"] + 1) * 64].tobytes().hex() == r["bytes"]
    assert [r["row"] for r in c["rows"]] == [0, 1, 262139 // 2, 262138]


def test_model_items_at_real_size(fx, cache0):
    words = M.words(cache0)
    idx = [r["index"] for r in fx["items"]]
    assert idx == [0, 1, 262138, 262139, 262140, 8388607, 16777185]
    got = M.dataset_item(words, idx)
    for k, r in enumerate(fx["items"]):
        assert np.ascontiguousarray(got[k].astype("<u4")).view(np.uint8).tobytes().hex() == r["bytes"], r["index"]


def test_model_light_at_real_size(fx, cache0):
    """4 of the 16 block-0 rows (nonces 0, 2^32 - 1, 2^32 and 2^64 - 1 among them)"""
    words = M.words(cache0)
    pick = [fx["light"]["0"][k] for k in (0, 2, 3, 4)]
    assert [r["nonce"] for r in pick] == [0, 2**32 - 1, 2**32, 2**64 - 1]
    h, n, mix, res = _rows(pick)
    d, r = M.hashimoto_light(1073739904, words, h, n)
    assert (d == mix).all() and (r == res).all()


# ---------------------------------------------------------------- ABI pins
def test_abi_pins():
    from gsv import _lib
    from gsv import ethash as E
    txt = open(os.path.join(ROOT, "include", "gsv.h")).read()

    def val(name):
        return int(re.search(r"#define %s (\d+)" % name, txt).group(1))
    assert val("GSV_ST_INVALID_DIFFICULTY") == _lib.ST_INVALID_DIFFICULTY == 16
    assert val("GSV_ST_INVALID_MIX_DIGEST") == _lib.ST_INVALID_MIX_DIGEST == 17
    assert val("GSV_ST_INVALID_POW") == _lib.ST_INVALID_POW == 18
    for st in (16, 17, 18):
        assert st in _lib.STATUS_STRINGS
    assert val("GSV_K_ETHASH_ITEMS") == _lib.K_ETHASH_ITEMS == 18
    assert val("GSV_K_ETHASH_LIGHT") == _lib.K_ETHASH_LIGHT == 19
    assert val("GSV_K_TOP") == _lib.K_TOP == 20
    assert val("GSV_K_CAP") == 18
    assert val("GSV_ETHASH_MAX_CACHES") == _lib.ETHASH_MAX_CACHES == 3
    assert E.cacheSize(0) == 16776896 and E.datasetSize(0) == 1073739904


def test_sizes_and_seeds_through_the_library(fx):
    from gsv import ethash as E
    for s in fx["sizes"]:
        assert E.cacheSize(s["block"]) == s["cache_size"]
        assert E.datasetSize(s["block"]) == s["dataset_size"]
        assert E.seedHash(s["block"]).hex() == s["seed"]
    # epochs past the reference's tables follow the same formula: a prime row count below the linear bound
    e = 2048
    size = E.cacheSize(e * 30000)
    assert size % 64 == 0 and size <= (1 << 24) + (1 << 17) * e - 64
    rows = size // 64
    assert all(rows % f for f in range(2, int(rows ** 0.5) + 1))


def test_host_entry_points_check_their_arguments():
    from gsv import _lib
    L = _lib.load()
    out = (ctypes.c_uint8 * 128)()
    seed = (ctypes.c_uint8 * 32)()
    assert L.gsv_ethash_seed_hash(0, None) == _lib.E_INVALID_ARG
    assert L.gsv_ethash_make_cache(None, 64, out) == _lib.E_INVALID_ARG
    assert L.gsv_ethash_make_cache(seed, 0, out) == _lib.E_INVALID_ARG
    assert L.gsv_ethash_make_cache(seed, 100, out) == _lib.E_INVALID_ARG
    assert L.gsv_ethash_make_cache(seed, 128, out) == 0
    assert L.gsv_ctx_ethash_caches(None, None) == _lib.E_INVALID_ARG
    assert L.gsv_ethash_light_batch(None, None, 0, None, None, 1, None, None) == _lib.E_INVALID_ARG
    assert L.gsv_ethash_dataset_items_dev(None, None, 64, 0, 1, None, None) == _lib.E_INVALID_ARG
