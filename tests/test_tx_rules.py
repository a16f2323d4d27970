"""The transaction decode and signer rules of the reference, checked against an independent model.

The notary path's RLP reader exists in three copies (oracle/gsv_oracle.c tx_decode, csrc/tx_host.hip
tx_prepare, csrc/notary.hip k_notary_tx) written from one reading of rlp/decode.go; a misreading they
share cannot fail a test that compares one copy with another.  tests/tx_rules_model.py is written from the
Go text instead and is pinned here to the reference's own vectors (tests/golden/rlp_rules.json: rows of
rlp/decode_test.go; tests/golden/tx.json).  The oracle and the host decoder are then compared with it on
the structured corpus of tests/tx_rules_corpus.py: status, sender and sighash (oracle); status, preimage
hash, r, s, v and vbig (host).  CPU-only; tests/test_gpu_tx_rules.py runs the same corpus on the GPU."""
import pytest

import tx_rules_corpus as C
import tx_rules_model as M
from conftest import golden
from test_tx_host import prepare, txh  # noqa: F401  (the host decoder's harness and its fixture)


# ---------------------------------------------------------------- the model against the reference's vectors
def _run_rule(row):
    s = M.Stream(bytes.fromhex(row["input"]), "len" if row.get("limited", True) else None)
    dec = row["decoder"]
    if dec == "uint":
        return M.decode_uint(s, row.get("bits", 64))
    if dec == "bytes":
        return M.decode_bytes(s).hex()
    if dec == "bigint":
        return M.decode_bigint(s)
    if dec == "bytearray":
        return M.decode_byte_array(s, row["array_len"]).hex()
    if dec == "address-or-nil":
        v = M.decode_optional_byte_array(s, row["array_len"])
        return None if v is None else v.hex()
    if dec == "list":
        return s.List()
    raise AssertionError(dec)


def test_model_reproduces_rlp_decode_test_rows():
    rows = golden("rlp_rules.json")["rows"]
    assert {r["decoder"] for r in rows} >= {"uint", "bytes", "bigint", "address-or-nil", "list"}
    for row in rows:
        try:
            got = ("ok", _run_rule(row))
        except M.RLPError as e:
            got = ("error", e.name)
        want = ("ok", row["ok"]) if "ok" in row else ("error", row["error"])
        assert got == want, (row, got)


def _final(oracle, d):
    """the model's ST_OK verdict finished by the curve recovery"""
    sig = d["r"].to_bytes(32, "big") + d["s"].to_bytes(32, "big") + bytes([d["v"]])
    rc, pub = oracle.ecrecover(oracle.keccak256(d["pre"]), sig)
    return oracle.keccak256(pub[1:])[12:] if rc == 1 else None


def test_model_reproduces_tx_vectors(oracle):
    g = golden("tx.json")
    for v in g["eip155_chain1"]:
        st, d = M.tx_verdict(bytes.fromhex(v["rlp"]), M.SIGNER_EIP155, 1)
        assert st == M.ST_OK and _final(oracle, d).hex() == v["addr"], v
        assert M.tx_verdict(bytes.fromhex(v["rlp"]), M.SIGNER_EIP155, 2)[0] == M.ST_INVALID_CHAIN_ID
    for v in g["homestead"]:
        st, d = M.tx_verdict(bytes.fromhex(v["rlp"]), M.SIGNER_HOMESTEAD, 1)
        assert st == M.ST_OK and _final(oracle, d).hex() == v["addr"], v
    for v in g["homestead_sighash"]:
        st, d = M.tx_verdict(bytes.fromhex(v["rlp"]), M.SIGNER_HOMESTEAD, 1)
        assert "pre" in d and oracle.keccak256(d["pre"]).hex() == v["sighash"], v


def test_model_blob_codec_roundtrip_and_edges():
    blobs = [b"\x01", bytes(range(31)), bytes(range(32)), bytes(200)]
    body = M.serialize(blobs, [0, 1, 0, 1])
    assert M.deserialize(body) == [(b, bool(k % 2)) for k, b in enumerate(blobs)]
    # indicator & 0x1F is the length, bits 5/6 are ignored, a partial chunk and trailing non-terminal
    # chunks are dropped (marshal.go:132-134, :145, :150-166)
    body = bytes([0x62]) + b"ab" + bytes(29) + bytes(32) + bytes(17)
    assert M.deserialize(body) == [(b"ab", False)]


# ---------------------------------------------------------------- corpus
@pytest.fixture(scope="module")
def corpora(oracle):
    return {cid: C.build(oracle, cid) for cid in C.CHAIN_IDS}


def _oracle_verdict(oracle, blob, cid, signer):
    st, addr = oracle.tx_sender(blob, cid, signer)
    return st, (addr.hex() if addr else None)


def _host_verdict(L, blob, cid, signer):
    st, pre, rs, v, vbig = prepare(L, blob, cid, signer)
    return (st, vbig) if st == 0 else (st,)


def _report(bad, n=4):
    return "%d disagreements; first %d:\n" % (len(bad), min(n, len(bad))) + "\n".join(
        "%s\n  blob %s\n  model %s\n  oracle %s\n  host %s" % b for b in bad[:n])


def _coverage(cases_exp, oracle):
    """every status occurs, and every positive case is ST_OK with the signing key's address"""
    seen, addr = set(), C.key_address(oracle)
    for cases, exp, signer in cases_exp:
        seen |= {e[0] for e in exp}
        pos = [(c, e) for c, e in zip(cases, exp) if C.positive_ok(c, signer)]
        assert len(pos) >= 20
        for c, e in pos:
            assert e[0] == M.ST_OK and e[1] == addr, (c.label, e[0])
    assert seen >= C.ALL_STATUSES, seen


def test_oracle_matches_model_on_corpus(oracle, corpora, txh):  # noqa: F811
    """oracle.tx_sender (status, sender) and oracle.tx_sighash against the model, every case, all three
    signers, chain ids 0, 1 and 2^63 + 5."""
    bad, cov = [], []
    for cid, cases in corpora.items():
        for signer in C.SIGNERS:
            exp = C.expected(oracle, cases, cid, signer)
            cov.append((cases, exp, signer))
            for c, (st, addr, d) in zip(cases, exp):
                ost, oaddr = oracle.tx_sender(c.blob, cid, signer)
                hst, sh = oracle.tx_sighash(c.blob, cid, signer)
                ok = ost == st and (st != M.ST_OK or oaddr == addr)
                if st == M.ST_BAD_RLP:
                    ok = ok and hst == M.ST_BAD_RLP
                else:  # oracle_tx_sighash hashes with the chain id whenever the signer is EIP155
                    pre = M.sighash_preimage(d["tx"], cid if signer == M.SIGNER_EIP155 else None)
                    ok = ok and hst == 0 and sh == oracle.keccak256(pre)
                if not ok:
                    bad.append(("%s (chain id %d, signer %d)" % (c.label, cid, signer), c.blob.hex(),
                                (st, addr.hex() if addr else d.get("error")),
                                _oracle_verdict(oracle, c.blob, cid, signer) + (hst,),
                                _host_verdict(txh, c.blob, cid, signer)))
    assert not bad, _report(bad)
    _coverage(cov, oracle)


def test_host_decoder_matches_model_on_corpus(oracle, corpora, txh):  # noqa: F811
    """tx_prepare against the model: status, Keccak of the preimage, r, s, v and vbig.  The host decoder
    reports what it can see before the recovery: ST_BAD_RLP, ST_INVALID_CHAIN_ID, ST_INVALID_SIG for a
    negative V - 2*chainId - 8, else ST_OK with vbig set when V', R or S cannot pass recoverPlain's and
    ValidateSignatureValues' width checks (the kernel then reports ST_INVALID_SIG)."""
    bad, cov = [], []
    for cid, cases in corpora.items():
        for signer in C.SIGNERS:
            exp = C.expected(oracle, cases, cid, signer)
            cov.append((cases, exp, signer))
            for c, (st, addr, d) in zip(cases, exp):
                hst, pre, rs, v, vbig = prepare(txh, c.blob, cid, signer)
                if st in (M.ST_BAD_RLP, M.ST_INVALID_CHAIN_ID):
                    ok = hst == st
                elif d["vprime"] < 0:
                    ok = hst == M.ST_INVALID_SIG
                else:
                    wide = d["r"].bit_length() > 256 or d["s"].bit_length() > 256
                    ok = (hst == M.ST_OK and pre == d["pre"] and v == d["vprime"] & M.U64 and
                          vbig == int(wide or d["vprime"].bit_length() > 8))
                    if ok and not wide:
                        ok = rs == d["r"].to_bytes(32, "big") + d["s"].to_bytes(32, "big")
                    if ok and vbig:
                        ok = st == M.ST_INVALID_SIG
                if not ok:
                    bad.append(("%s (chain id %d, signer %d)" % (c.label, cid, signer), c.blob.hex(),
                                (st, addr.hex() if addr else d.get("error"), d.get("vprime")),
                                _oracle_verdict(oracle, c.blob, cid, signer), (hst, v, vbig)))
    assert not bad, _report(bad)
    _coverage(cov, oracle)


def test_corpus_shape(corpora):
    """about two thousand blobs per chain id, each case as is and shifted (the generator itself fails
    where no padding puts a replaced item at a chunk's last byte)"""
    for cases in corpora.values():
        assert 1800 <= len(cases) <= 2600
        labels = [c.label for c in cases]
        assert len(set(labels)) == len(labels)
        assert sum("shifted" in l for l in labels) * 2 == len(labels)
