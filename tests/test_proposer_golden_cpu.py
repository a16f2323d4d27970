"""CPU checks of tests/golden/proposer_small.json: the file is what its generator derives from the oracle
today, and its values hang together (the body deserializes to the transactions, the signature recovers
the proposer)."""
import hashlib
import importlib.util
import os

from conftest import GOLDEN, golden


def _generator():
    spec = importlib.util.spec_from_file_location("make_proposer_golden", os.path.join(GOLDEN, "make_proposer_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_fixture_is_what_the_oracle_derives():
    assert _generator().build() == golden("proposer_small.json")


def test_fixture_hangs_together(oracle):
    g = golden("proposer_small.json")["collations"]
    assert [c["name"] for c in g] == ["eip155_chain1", "homestead", "empty"]
    assert [len(c["txs"]) for c in g] == [10, 2, 0]
    for c in g:
        txs = [bytes.fromhex(t) for t in c["txs"]]
        body = oracle.blob_serialize(txs) if txs else b""
        assert len(body) == c["body_len"] and hashlib.sha256(body).hexdigest() == c["body_sha256"]
        assert oracle.blob_deserialize(body) == [(t, 0) for t in txs]
        for t, a in zip(txs, c["senders"]):
            assert oracle.tx_sender(t, 1, 0) == (0, bytes.fromhex(a))
        rc, pub = oracle.ecrecover(bytes.fromhex(c["hash"]), bytes.fromhex(c["sig"]))
        assert rc == 1 and oracle.keccak256(pub[1:])[12:].hex() == c["proposer"]
    assert g[2]["chunk_root"] == "56e81f171bcc55a6ff8345e692c0f86e5b48e01b996cadc001622fb5e363b421"
    assert os.path.getsize(os.path.join(GOLDEN, "proposer_small.json")) < 64 << 10
