"""Generates tests/golden/secp_sign.json: recorded crypto.Sign results (run where the reference build
oracle/_ref exists; the tests only read the JSON).

  rows  64 x {key, msg, sig, pub}: sig = the reference's secp256k1_ecdsa_sign_recoverable with
        secp256k1_nonce_function_rfc6979 (gsvref_sign), pub = its secp256k1_ec_pubkey_create
        (gsvref_pubkey).  The edge rows come first (tests/rfc6979_model.py edge_pairs: keys 1, n - 1, ...
        against messages 0, n - 1, n, n + 1, 2^256 - 1, ...), seeded random rows fill up to 64.

    python tests/golden/make_secp_sign.py
"""
from __future__ import annotations

import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import rfc6979_model as M  # noqa: E402
from oracle import oracle as O  # noqa: E402

SEED = 6979
ROWS = 64


def main():
    R = O.ref()
    assert R is not None, "the reference build (make -C oracle ref) is needed"
    pairs = M.edge_pairs()
    pairs += M.random_pairs(ROWS - len(pairs), SEED)
    rows = []
    for key, msg in pairs:
        sig = ctypes.create_string_buffer(65)
        pub = ctypes.create_string_buffer(65)
        assert R.gsvref_sign(sig, msg, key) == 1 and R.gsvref_pubkey(pub, key) == 1
        rows.append({"key": key.hex(), "msg": msg.hex(), "sig": sig.raw.hex(), "pub": pub.raw.hex()})
    with open(os.path.join(HERE, "secp_sign.json"), "w") as f:
        json.dump({"source": "gsvref_sign / gsvref_pubkey (oracle/ref_shim.c) over the reference's libsecp256k1",
                   "seed": SEED, "rows": rows}, f, indent=1)
        f.write("\n")
    print("wrote secp_sign.json:", len(rows), "rows, recids", sorted({r["sig"][-2:] for r in rows}))


if __name__ == "__main__":
    main()
