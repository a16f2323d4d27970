"""Writes tests/golden/proposer_small.json: three collations as proposer.createCollation builds them
(sharding/proposer/proposer.go:55-92), every value from the CPU oracle.

    python tests/golden/make_proposer_golden.py

Collations: the ten EIP-155 vectors, the Homestead vectors (both from tests/golden/tx.json) and an empty
transaction list.  Keys and header fields are fixed below; the proposer address is the key's own.  Per
collation: SHA-256 of the body (utils.Serialize of the encoded transactions), the chunk root, the hash of
the header with ProposerSignature empty and the signature over it: the oracle's ECDSA with RFC 6979's
nonce from tests/rfc6979_model.py, cross-checked against the reference build's signer where that is
built.  tests/test_proposer_golden_cpu.py re-derives the file from build(), so it cannot drift."""
import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

KEYS = ["45a915e4d060149eb4365960e6a7a45f334393093061116b197e3240065ff2d8",  # core/types tests' key
        "00000000000000000000000000000000000000000000000000000000000000a5",
        "fffffffffffffffffffffffffffffffebaaedce6af48a03bbfd25e8cd0364140"]  # n - 1
SHARDS = [1, 99, 0]
PERIODS = [7, 128, 0x0123456789ABCDEF0123]


def build():
    from oracle import oracle as O
    import rfc6979_model as M
    tx = json.load(open(os.path.join(HERE, "tx.json")))
    lists = [("eip155_chain1", tx["eip155_chain1"]), ("homestead", tx["homestead"]), ("empty", [])]
    R = O.ref()
    out = []
    for (name, rows), key, sid, per in zip(lists, KEYS, SHARDS, PERIODS):
        key = bytes.fromhex(key)
        txs = [bytes.fromhex(r["rlp"]) for r in rows]
        body = O.blob_serialize(txs) if txs else b""
        root = O.derive_sha_bytes(body)
        prop = O.keccak256(O.secp_pubkey(key)[1:])[12:]
        h = O.collation_header_hash(sid, root, per, prop, None)
        sig = O.secp_sign(h, key, M.nonce(key, h))
        if R is not None:
            ref = ctypes.create_string_buffer(65)
            assert R.gsvref_sign(ref, h, key) == 1 and ref.raw == sig, name
        out.append({"name": name, "txs": [t.hex() for t in txs], "senders": [r["addr"] for r in rows],
                    "shard_id": sid, "period": per, "proposer": prop.hex(), "key": key.hex(),
                    "body_len": len(body), "body_sha256": hashlib.sha256(body).hexdigest(),
                    "chunk_root": root.hex(), "hash": h.hex(), "sig": sig.hex(),
                    "signed_hash": O.collation_header_hash(sid, root, per, prop, sig).hex()})
    return {"collations": out}


if __name__ == "__main__":
    with open(os.path.join(HERE, "proposer_small.json"), "w") as f:
        json.dump(build(), f, indent=1)
        f.write("\n")
