"""Generates tests/golden/ethash.json: recorded results of the reference's C implementation of ethash
(vendored libethash).  Run by hand where a checkout of the reference is at hand:

    python tests/golden/make_ethash.py --reference <root of the reference checkout>

It compiles libethash's internal.c, sha3.c, io.c and io_posix.c straight from the reference's vendor
directory into a temporary directory, with the small driver below, and records what the driver prints.
Nothing is compiled into the repository.  Before it writes, it checks the build against the reference's own
Go vectors: TestHashimoto's digest and result, and the hex literals of TestCacheGeneration /
TestDatasetGeneration (consensus/ethash/algorithm_test.go), which must contain the driver's test-mode caches
and dataset.

What it records (tests/test_ethash_cpu.py, tests/test_gpu_ethash.py):
  sizes        cache size, dataset size and seed hash for six block numbers; the Keccak-256 of all 2,048
               cache sizes and of all 2,048 dataset sizes as little-endian u64
  caches       epochs 0 and 1: Keccak-256 of the whole cache and rows 0, 1, rows / 2, rows - 1
  items        epoch-0 dataset items at seven indices (ethash_calculate_dag_item)
  light        16 (hash, nonce, mix, result) rows at block 0 and 8 at block 30,000 (ethash_light_compute)
  test_mode    the two 1,024-byte caches, the Keccak-256 of the 32 KiB dataset, 32 light rows, the Go vector
"""
import argparse
import json
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
LIBETHASH = "vendor/github.com/ethereum/ethash/src/libethash"
GO_TEST = "consensus/ethash/algorithm_test.go"

GO_HASH = "c9149cc0386e689d789a1c2f3d5d169a61a6218ed30e74414dc736e442ef3d1f"
GO_DIGEST = "e4073cffaef931d37117cefd9afd27ea0f1cad6a981dd2605c4a1ac97c519800"
GO_RESULT = "d3539235ee2e6f8db665c0a72169f55b7f6c605712330b778ec3944f0eb5a557"
MIX_BLOCK0_NONCE19 = "827f14fcecf8cdea1a71c3f80b286b7f2048205ead02c2ef404c0226a80e5aac"

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ethash.h"
#include "internal.h"
#include "sha3.h"

static void hex(const char* key, const void* p, size_t n) {
    const uint8_t* b = (const uint8_t*)p;
    printf("%s ", key);
    for (size_t i = 0; i < n; i++) printf("%02x", b[i]);
    printf("\n");
}

static const uint64_t NONCES[8] = {0ull, 1ull, 0xFFFFFFFFull, 0x100000000ull, 0xFFFFFFFFFFFFFFFFull, 19ull,
                                   0x0123456789ABCDEFull, 0x8000000000000000ull};

/* hash k of a series: Keccak-256("gsv ethash" tag k) */
static ethash_h256_t series_hash(int tag, int k) {
    char msg[64];
    ethash_h256_t h;
    int n = snprintf(msg, sizeof msg, "gsv ethash %d %d", tag, k);
    SHA3_256(&h, (const uint8_t*)msg, (size_t)n);
    return h;
}

static uint64_t series_nonce(int tag, int k) {
    if (k < 8) return NONCES[k];
    ethash_h256_t h = series_hash(tag + 1000, k);
    uint64_t v;
    memcpy(&v, &h, 8);
    return v;
}

static void light_rows(const char* key, ethash_light_t light, uint64_t full_size, int tag, int count) {
    for (int k = 0; k < count; k++) {
        ethash_h256_t h = series_hash(tag, k);
        uint64_t nonce = series_nonce(tag, k);
        ethash_return_value_t r = ethash_light_compute_internal(light, full_size, h, nonce);
        if (!r.success) exit(2);
        printf("%s %llu ", key, (unsigned long long)nonce);
        for (int i = 0; i < 32; i++) printf("%02x", h.b[i]);
        printf(" ");
        for (int i = 0; i < 32; i++) printf("%02x", r.mix_hash.b[i]);
        printf(" ");
        for (int i = 0; i < 32; i++) printf("%02x", r.result.b[i]);
        printf("\n");
    }
}

static void cache_rows(const char* key, ethash_light_t light) {
    uint32_t rows = (uint32_t)(light->cache_size / 64);
    uint32_t pick[4] = {0, 1, rows / 2, rows - 1};
    ethash_h256_t d;
    SHA3_256(&d, (const uint8_t*)light->cache, (size_t)light->cache_size);
    printf("%s_digest ", key);
    for (int i = 0; i < 32; i++) printf("%02x", d.b[i]);
    printf("\n");
    for (int k = 0; k < 4; k++) {
        printf("%s_row %u ", key, pick[k]);
        const uint8_t* p = (const uint8_t*)light->cache + (size_t)pick[k] * 64;
        for (int i = 0; i < 64; i++) printf("%02x", p[i]);
        printf("\n");
    }
}

int main(void) {
    static const uint64_t BLOCKS[6] = {0, 29999, 30000, 60000, 3000000, 61439999};
    for (int k = 0; k < 6; k++) {
        ethash_h256_t s = ethash_get_seedhash(BLOCKS[k]);
        printf("size %llu %llu %llu ", (unsigned long long)BLOCKS[k],
               (unsigned long long)ethash_get_cachesize(BLOCKS[k]), (unsigned long long)ethash_get_datasize(BLOCKS[k]));
        for (int i = 0; i < 32; i++) printf("%02x", s.b[i]);
        printf("\n");
    }
    {
        static uint64_t cs[2048], ds[2048]; /* little-endian machine */
        for (uint64_t e = 0; e < 2048; e++) {
            cs[e] = ethash_get_cachesize(e * 30000);
            ds[e] = ethash_get_datasize(e * 30000);
        }
        ethash_h256_t d;
        SHA3_256(&d, (const uint8_t*)cs, sizeof cs);
        hex("cache_sizes_digest", &d, 32);
        SHA3_256(&d, (const uint8_t*)ds, sizeof ds);
        hex("dataset_sizes_digest", &d, 32);
    }
    /* full size, epochs 0 and 1 */
    ethash_light_t l0 = ethash_light_new(0);
    cache_rows("cache0", l0);
    {
        static const uint32_t IDX[7] = {0, 1, 262138, 262139, 262140, 8388607, 16777185};
        for (int k = 0; k < 7; k++) {
            node nd;
            ethash_calculate_dag_item(&nd, IDX[k], l0);
            printf("item %u ", IDX[k]);
            for (int i = 0; i < 64; i++) printf("%02x", nd.bytes[i]);
            printf("\n");
        }
    }
    light_rows("light0", l0, ethash_get_datasize(0), 0, 16);
    {
        ethash_h256_t h;
        const char* hx = "c9149cc0386e689d789a1c2f3d5d169a61a6218ed30e74414dc736e442ef3d1f";
        for (int i = 0; i < 32; i++) {
            unsigned v;
            sscanf(hx + 2 * i, "%2x", &v);
            h.b[i] = (uint8_t)v;
        }
        ethash_return_value_t r = ethash_light_compute(l0, h, 19);
        hex("check_block0_nonce19_mix", &r.mix_hash, 32);
        /* the Go vector: seed of zeros, 1,024-byte cache, 32 KiB dataset */
        ethash_h256_t zero;
        memset(&zero, 0, 32);
        ethash_light_t t0 = ethash_light_new_internal(1024, &zero);
        r = ethash_light_compute_internal(t0, 32 * 1024, h, 0);
        hex("go_digest", &r.mix_hash, 32);
        hex("go_result", &r.result, 32);
        hex("test_cache0", t0->cache, 1024);
        static uint8_t full[32 * 1024];
        if (!ethash_compute_full_data(full, sizeof full, t0, NULL)) exit(3);
        hex("test_dataset", full, sizeof full);
        ethash_h256_t d;
        SHA3_256(&d, full, sizeof full);
        hex("test_dataset_digest", &d, 32);
        light_rows("test_light", t0, 32 * 1024, 2, 32);
        ethash_h256_t s1 = ethash_get_seedhash(30000);
        ethash_light_t t1 = ethash_light_new_internal(1024, &s1);
        hex("test_cache1", t1->cache, 1024);
        ethash_light_delete(t0);
        ethash_light_delete(t1);
    }
    ethash_light_delete(l0);
    ethash_light_t l1 = ethash_light_new(30000);
    cache_rows("cache1", l1);
    light_rows("light1", l1, ethash_get_datasize(30000), 1, 8);
    ethash_light_delete(l1);
    return 0;
}
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    args = ap.parse_args()
    src = os.path.join(args.reference, LIBETHASH)
    with tempfile.TemporaryDirectory() as tmp:
        drv = os.path.join(tmp, "driver.c")
        with open(drv, "w") as f:
            f.write(DRIVER)
        exe = os.path.join(tmp, "driver")
        subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-I", src, "-o", exe, drv] +
                              [os.path.join(src, n) for n in ("internal.c", "sha3.c", "io.c", "io_posix.c")] + ["-lm"])
        lines = subprocess.check_output([exe], cwd=tmp).decode().splitlines()

    rec = {"source": "libethash (ethash_light_compute, ethash_calculate_dag_item, ethash_get_cachesize / _datasize / "
                     "_seedhash) of the reference's vendor tree, gcc -O2; see tests/golden/make_ethash.py",
           "sizes": [], "caches": {"0": {"rows": []}, "1": {"rows": []}}, "items": [], "light": {"0": [], "30000": []},
           "test_mode": {"light": []}}
    raw = {}
    for ln in lines:
        p = ln.split()
        if p[0] == "size":
            rec["sizes"].append({"block": int(p[1]), "cache_size": int(p[2]), "dataset_size": int(p[3]), "seed": p[4]})
        elif p[0] in ("cache0_digest", "cache1_digest"):
            rec["caches"][p[0][5]]["digest"] = p[1]
        elif p[0] in ("cache0_row", "cache1_row"):
            rec["caches"][p[0][5]]["rows"].append({"row": int(p[1]), "bytes": p[2]})
        elif p[0] == "item":
            rec["items"].append({"index": int(p[1]), "bytes": p[2]})
        elif p[0] in ("light0", "light1", "test_light"):
            row = {"nonce": int(p[1]), "hash": p[2], "mix": p[3], "result": p[4]}
            (rec["test_mode"]["light"] if p[0] == "test_light" else
             rec["light"]["0" if p[0] == "light0" else "30000"]).append(row)
        else:
            raw[p[0]] = p[1]

    # the build against the reference's own vectors
    assert raw["go_digest"] == GO_DIGEST and raw["go_result"] == GO_RESULT, "TestHashimoto vector"
    assert raw["check_block0_nonce19_mix"] == MIX_BLOCK0_NONCE19
    go = open(os.path.join(args.reference, GO_TEST)).read().replace('" +\n', "").replace('"', "")
    go = "".join(go.split())
    for key in ("test_cache0", "test_cache1", "test_dataset"):
        assert raw[key] in go, key + " is not among the Go test's literals"

    rec["cache_sizes_digest"] = raw["cache_sizes_digest"]
    rec["dataset_sizes_digest"] = raw["dataset_sizes_digest"]
    rec["test_mode"].update({"cache_bytes": 1024, "dataset_bytes": 32 * 1024, "cache0": raw["test_cache0"],
                             "cache1": raw["test_cache1"], "dataset_digest": raw["test_dataset_digest"],
                             "go": {"hash": GO_HASH, "nonce": 0, "digest": GO_DIGEST, "result": GO_RESULT}})
    out = os.path.join(HERE, "ethash.json")
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
