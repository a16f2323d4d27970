"""Generates tests/golden/block_headers.json: two real sealed headers of the reference's own tests with their
expectations, and chains built with the model (tests/block_header_model.py).  Run by hand where a checkout of the
reference is at hand and the oracle is built:

    python tests/golden/make_block_headers.py --reference <root of the reference checkout>

The reference is read for two things only.  (1) The two headers: the 508-byte header inside blockEnc of
core/types/block_test.go (its Hash is pinned there) and the fields of mainnet block 3,311,058 in
consensus/ethash/algorithm_test.go, for which the reference asserts VerifySeal == nil.  (2) The seal of each, run
once through the reference's libethash (compiled into a temporary directory with the small driver below, as
tests/golden/make_ethash.py does): the recorded verdict is whatever that run gives.  Nothing is compiled into the
repository.

What it records (tests/test_block_header_cpu.py, tests/test_gpu_block_header.py):
  reference   the two headers: RLP, Hash, HashNoNonce, libethash's mix digest and result, the seal's status
  chain40     a parent and 40 headers under TestChainConfig (every fork at block 0), a handful of them sealed in
              test mode by the numpy ethash model (tests/ethash_model.py) over the 1,024-byte epoch-0 cache
  forks       a parent and 16 headers across Frontier -> Homestead -> Byzantium under a configuration with the forks
              at small numbers, the DAO window pro-fork, and an EIP-150 hash header
  forks_no_dao    the same numbers under the no-fork configuration
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]

import block_header_model as B  # noqa: E402
import ethash_model as M  # noqa: E402

LIBETHASH = "vendor/github.com/ethereum/ethash/src/libethash"
BLOCK1_HASH = "0a5843ac1cb04865017cb35a57b50b07084e5fcee39b5acadade33149f4fff9e"  # block_test.go:49

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include "ethash.h"

/* argv: block number, 64 hex digits of the hash without nonce, the nonce */
int main(int argc, char** argv) {
    if (argc != 4) return 1;
    ethash_h256_t h;
    for (int i = 0; i < 32; i++) {
        unsigned v;
        sscanf(argv[2] + 2 * i, "%2x", &v);
        h.b[i] = (uint8_t)v;
    }
    ethash_light_t light = ethash_light_new(strtoull(argv[1], NULL, 10));
    ethash_return_value_t r = ethash_light_compute(light, h, strtoull(argv[3], NULL, 10));
    if (!r.success) return 2;
    for (int i = 0; i < 32; i++) printf("%02x", r.mix_hash.b[i]);
    printf(" ");
    for (int i = 0; i < 32; i++) printf("%02x", r.result.b[i]);
    printf("\n");
    ethash_light_delete(light);
    return 0;
}
"""


def reference_headers(ref):
    go = open(os.path.join(ref, "core/types/block_test.go")).read()
    enc = bytes.fromhex(re.search(r'blockEnc := common.FromHex\("([0-9a-f]+)"\)', go).group(1))
    assert enc[:3] == bytes.fromhex("f90260") and enc[3:6] == bytes.fromhex("f901f9")
    block1 = enc[3:3 + 3 + 0x1F9]
    assert len(block1) == 508 and B.header_hash(block1).hex() == BLOCK1_HASH
    go = open(os.path.join(ref, "consensus/ethash/algorithm_test.go")).read()
    at = go.index("big.NewInt(3311058)")
    txt = go[at - 200:at + 1400]

    def hx(name):
        return bytes.fromhex(re.search(name + r':\s+common\.Hex\w+\("0x([0-9a-f]+)"\)', txt).group(1))

    def num(name):
        return int(re.search(name + r":\s+(?:big\.NewInt\()?(\d+)", txt).group(1))
    h = B.new_header(ParentHash=hx("ParentHash"), UncleHash=hx("UncleHash"), Coinbase=hx("Coinbase"), Root=hx("Root"),
                     TxHash=hx("TxHash"), ReceiptHash=hx("ReceiptHash"), Difficulty=num("Difficulty"),
                     Number=num("Number"), GasLimit=num("GasLimit"), GasUsed=num("GasUsed"), Time=num("Time"),
                     Extra=re.search(r'Extra:\s+\[\]byte\("([^"]+)"\)', txt).group(1).encode(), MixDigest=hx("MixDigest"),
                     Nonce=int(re.search(r"EncodeNonce\(0x([0-9a-f]+)\)", txt).group(1), 16).to_bytes(8, "big"))
    assert h["Number"] == 3311058 and h["Difficulty"] == 167925187834220
    return block1, B.encode_header(h)


def seal_rows(ref, blobs):
    src = os.path.join(ref, LIBETHASH)
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        drv = os.path.join(tmp, "driver.c")
        with open(drv, "w") as f:
            f.write(DRIVER)
        exe = os.path.join(tmp, "driver")
        subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-I", src, "-o", exe, drv] +
                              [os.path.join(src, n) for n in ("internal.c", "sha3.c", "io.c", "io_posix.c")] + ["-lm"])
        for blob in blobs:
            h = B.decode_header(blob)
            hnn = B.hash_no_nonce(h)
            mix, res = subprocess.check_output([exe, str(h["Number"]), hnn.hex(), str(B.nonce_number(h))],
                                               cwd=tmp).decode().split()
            # VerifySeal's checks in its order (consensus.go:477-499)
            if h["Difficulty"] <= 0:
                st = B.ST_INVALID_DIFFICULTY
            elif bytes.fromhex(mix) != h["MixDigest"]:
                st = B.ST_INVALID_MIX_DIGEST
            elif int(res, 16) > ((1 << 256) - 1) // h["Difficulty"]:
                st = B.ST_INVALID_POW
            else:
                st = B.ST_OK
            rows.append({"rlp": blob.hex(), "number": h["Number"], "hash": B.header_hash(blob).hex(),
                         "hash_no_nonce": hnn.hex(), "nonce": B.nonce_number(h), "mix": mix, "result": res,
                         "seal_status": st})
    return rows


class Sealer:
    """the test-mode seal of epoch 0: the 1,024-byte cache of tests/golden/ethash.json, a 32 KiB dataset"""

    def __init__(self):
        fx = json.load(open(os.path.join(HERE, "ethash.json")))
        cache = np.frombuffer(bytes.fromhex(fx["test_mode"]["cache0"]), np.uint8)
        self.dataset = M.dataset_item(M.words(cache), np.arange(512, dtype=np.uint32))

    def seal(self, h, start):
        hnn = np.frombuffer(B.hash_no_nonce(h), np.uint8)
        target = ((1 << 256) - 1) // h["Difficulty"]
        step = 1 << 15
        while True:
            nonces = np.uint64(start) + np.arange(step, dtype=np.uint64)
            d, r = M.hashimoto_full(32 * 1024, self.dataset, np.tile(hnn, (step, 1)), nonces)
            # a result within the target starts with at least 15 zero bits here: look at those rows only
            for k in np.nonzero(r[:, 0] == 0)[0]:
                if int.from_bytes(r[k].tobytes(), "big") <= target:
                    h["MixDigest"] = d[k].tobytes()
                    h["Nonce"] = int(nonces[k]).to_bytes(8, "big")
                    return
            start += step


def build_chain(cfg, parent, count, rng, dts, extras=None, sealed=(), sealer=None, gas_step=0):
    """`count` valid headers behind `parent` (a dict): header k has Time = parent.Time + dts[k % len(dts)]"""
    blobs, prev, prev_blob = [], parent, B.encode_header(parent)
    for k in range(count):
        h = B.new_header(ParentHash=B.header_hash(prev_blob), Coinbase=rng.bytes(20), Root=rng.bytes(32),
                         TxHash=rng.bytes(32), ReceiptHash=rng.bytes(32), Bloom=rng.bytes(256), Number=prev["Number"] + 1,
                         Time=prev["Time"] + dts[k % len(dts)], GasLimit=prev["GasLimit"] + gas_step,
                         Extra=rng.bytes(int(rng.integers(0, 33))), MixDigest=rng.bytes(32), Nonce=rng.bytes(8))
        if k % 3 == 1:
            h["UncleHash"] = rng.bytes(32)
        h["GasUsed"] = int(rng.integers(0, h["GasLimit"] + 1))
        if extras and h["Number"] in extras:
            h["Extra"] = extras[h["Number"]]
        h["Difficulty"] = B.calc_difficulty(cfg, h["Time"], prev)
        if k in sealed:
            sealer.seal(h, int(rng.integers(0, 1 << 62)))
        blob = B.encode_header(h)
        blobs.append(blob)
        prev, prev_blob = h, blob
    return blobs


def cfg_json(cfg):
    return {"homestead": cfg.homestead, "dao": cfg.dao, "dao_support": cfg.dao_support, "eip150": cfg.eip150,
            "eip150_hash": cfg.eip150_hash.hex(), "byzantium": cfg.byzantium}


def chain_json(cfg, parent, blobs, now, sealed=()):
    st, wants = B.verify_headers(cfg, blobs, B.encode_header(parent), now)
    assert st == [0] * len(blobs), st
    return {"config": cfg_json(cfg), "now": now, "parent": B.encode_header(parent).hex(),
            "headers": [b.hex() for b in blobs], "sealed": list(sealed),
            "hash": [B.header_hash(b).hex() for b in blobs],
            "hash_no_nonce": [B.hash_no_nonce(B.decode_header(b)).hex() for b in blobs],
            "difficulty": [B.decode_header(b)["Difficulty"] for b in blobs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    args = ap.parse_args()
    rec = {"source": "tests/golden/make_block_headers.py: two headers of the reference's tests with their seal run "
                     "through the reference's libethash (gcc -O2), and chains built with tests/block_header_model.py"}
    rec["reference"] = seal_rows(args.reference, reference_headers(args.reference))
    assert rec["reference"][0]["hash"] == BLOCK1_HASH
    assert rec["reference"][1]["seal_status"] == 0, "the reference asserts VerifySeal == nil for block 3,311,058"

    rng = np.random.default_rng(0xB10C)
    sealer = Sealer()
    # TestChainConfig: every fork at 0, so the Byzantium rule throughout; time steps on both sides of 9 and 18
    test_cfg = B.Config(homestead=0, eip150=0, byzantium=0)
    genesis = B.new_header(Difficulty=131072, Number=0, GasLimit=4712388, Time=1500000000, Extra=b"gsv")
    sealed = (0, 3, 17, 18, 39)
    dts = (10, 9, 14, 1, 18, 25, 8, 13, 40, 17)
    blobs = build_chain(test_cfg, genesis, 40, rng, dts, sealed=sealed, sealer=sealer, gas_step=1000)
    for k in sealed:
        assert B.decode_header(blobs[k])["Difficulty"] >= 131072
    rec["chain40"] = chain_json(test_cfg, genesis, blobs, 1500000000 + 40 * 40, sealed)

    # forks at small numbers: Frontier for 1, 2; Homestead from 3; the DAO window 5 .. 14; EIP-150 at 7; Byzantium
    # from 9
    parent = B.new_header(Difficulty=1 << 40, Number=0, GasLimit=8000000, Time=1438269988, UncleHash=rng.bytes(32))
    for key, support in (("forks", True), ("forks_no_dao", False)):
        cfg = B.Config(homestead=3, dao=5, dao_support=support, eip150=7, byzantium=9)
        extras = {n: B.DAO_EXTRA for n in range(5, 15)} if support else {5: b"dao-hard-fork!", 6: b"dao-hard-for"}
        blobs = build_chain(cfg, parent, 16, rng, (12, 13, 5, 30, 9, 1000, 11), extras=extras, gas_step=-7000)
        cfg.eip150_hash = B.header_hash(blobs[6])  # header 7
        rec[key] = chain_json(cfg, parent, blobs, 1438269988 + 16 * 1000)

    out = os.path.join(HERE, "block_headers.json")
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
