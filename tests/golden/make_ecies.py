"""Generates tests/golden/ecies.json from the Python model (tests/ecies_model.py); the tests regenerate it
and compare, so the file only pins the model's answers.

  good  rows of Encrypt: {tag, msg, pub, seckey (the recipient's), eph, iv, s2, ke, km, ct}: ct is what
        Encrypt makes of (msg, pub, eph, iv, s2) and what Decrypt under seckey opens.  Message lengths
        0 .. 1000 over every SHA-256 padding boundary of 64 + 16 + len and every AES partial block, s2 of
        0, 2, 7 and 64 bytes, and IVs whose counter carries (ecies_model.good_rows).  The row of length 0
        has status 14 and a zero ct: Encrypt refuses an empty message.
  bad   rows of Decrypt: {tag, ct, seckey, s2, status, msg}: one row at least for every numbered check
        of include/gsv.h (ecies_model.bad_rows); where the keys exist and the input has an IV and a tag,
        also ke, km
  Every row with ke / km also has sym_tag = HMAC-SHA256(km, em || s2) and sym_msg = the CTR decryption of
  em, whatever the row's own tag says: what the host build of the device headers must print.

    python tests/golden/make_ecies.py
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ecies_model as M  # noqa: E402


def _sym(row, ke, km, ct, s2):
    em = ct[65:-32]
    row.update(ke=ke.hex(), km=km.hex(), sym_tag=M.message_tag(km, em, s2).hex(),
               sym_msg=M.aes128_ctr(ke, em[:16], em[16:]).hex())


def fixture():
    good, bad = [], []
    for tag, msg, pub, sk, eph, iv, s2 in M.good_rows():
        st, ct = M.encrypt(msg, pub, eph, iv, s2)
        row = {"tag": tag, "msg": msg.hex(), "pub": pub.hex(), "seckey": sk.hex(), "eph": eph.hex(), "iv": iv.hex(),
               "s2": s2.hex(), "status": st, "ct": ct.hex()}
        if st == M.ST_OK:
            assert M.decrypt(ct, sk, s2) == (M.ST_OK, msg)
            ke, km = M.keys_of(pub, eph)
            _sym(row, ke, km, ct, s2)
            assert row["sym_tag"] == ct[-32:].hex() and row["sym_msg"] == msg.hex()
        good.append(row)
    for tag, ct, sk, s2, want in M.bad_rows():
        st, msg = M.decrypt(ct, sk, s2)
        assert st == want, tag
        row = {"tag": tag, "ct": ct.hex(), "seckey": sk.hex(), "s2": s2.hex(), "status": st, "msg": msg.hex()}
        if len(ct) >= M.OVERHEAD and ct[0] == 4 and M.E.ecdh(ct[1:65], sk)[0] == M.ST_OK:
            x, y = int.from_bytes(ct[1:33], "big"), int.from_bytes(ct[33:65], "big")
            if x < M.E.P and y < M.E.P:
                _sym(row, *M.keys_of(ct[1:65], sk), ct, s2)
        bad.append(row)
    return {"source": "tests/ecies_model.py", "seed": M.SEED, "good": good, "bad": bad}


def main():
    fx = fixture()
    path = os.path.join(HERE, "ecies.json")
    with open(path, "w") as f:
        json.dump(fx, f, indent=1)
        f.write("\n")
    st = [r["status"] for r in fx["bad"]]
    print("wrote ecies.json:", len(fx["good"]), "good rows,", len(fx["bad"]), "bad rows; statuses",
          {s: st.count(s) for s in sorted(set(st))}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
