"""Generates tests/golden/tx_sign.json: recorded types.SignTx results (run where the reference build
oracle/_ref exists; the tests only read the JSON).

  rows  {label, rlp, key, chain_id, signer, signed, hash, status}: the input, and what tests/tx_sign_model.py
        makes of it with the reference's own signer (gsvref_sign: secp256k1_ecdsa_sign_recoverable with
        secp256k1_nonce_function_rfc6979) and oracle.keccak256.  The first rows are found by a seeded search
        (tests/tx_sign_corpus.py find_short, at most 2^20 signatures): a 31-byte R, a 31-byte S, an R or S of at
        most 30 bytes.  Then every signer and chain id of the GPU differential over six transaction shapes,
        transactions that were signed before, and the failing classes.

    python tests/golden/make_tx_sign_golden.py
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import tx_sign_corpus as C  # noqa: E402
import tx_sign_model as S  # noqa: E402
from oracle import oracle as O  # noqa: E402


def main():
    sign = C.ref_signer(O)
    short = C.find_short(O)
    missing = [name for name, _ in C.SHORT_CLASSES if name not in short]
    assert not missing, "no transaction found within 2^20 signatures for: %s" % missing
    rows = []
    for label, blob, key, signer, cid in C.fixture_inputs(O, short):
        st, signed, h = S.sign_tx(blob, key, signer, cid, sign, O.keccak256)
        rows.append({"label": label, "rlp": blob.hex(), "key": key.hex(), "chain_id": hex(cid), "signer": signer,
                     "signed": signed.hex(), "hash": h.hex(), "status": st})
    with open(os.path.join(HERE, "tx_sign.json"), "w") as f:
        json.dump({"source": "tests/tx_sign_model.py with gsvref_sign (oracle/ref_shim.c) over the reference's "
                             "libsecp256k1 and oracle.keccak256", "rows": rows}, f, indent=1)
        f.write("\n")
    print("wrote tx_sign.json:", len(rows), "rows, statuses", sorted({r["status"] for r in rows}))


if __name__ == "__main__":
    main()
