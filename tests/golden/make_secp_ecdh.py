"""Generates tests/golden/secp_ecdh.json: recorded results of the reference's secp256k1_ext_scalar_mul
(run where the reference build oracle/_ref exists; the tests only read the JSON).

  rows  96 x {tag, point, scalar, ref_rc, ref_out, status, out, shared, keys48}
        ref_rc / ref_out  what the reference's function returned and left in its 64-byte point buffer
                          (untouched when ref_rc == 0), called through ctypes on oracle/_ref
        status            the library's expected status: 0, 11 (ST_INVALID_KEY) exactly where ref_rc == 0,
                          12 (ST_INVALID_CURVE) for a scalar in range with a point off the curve.  Those rows
                          record ref_rc == 1 and the reference's artefact in ref_out: the one divergence is
                          pinned here, not hidden
        out               the library's expected X || Y: ref_out where status == 0, else zero bytes
        shared, keys48    X, and Ke || Km by hashlib (tests/secp_ecdh_model.py kdf_keys); zero where failed
        The edge rows come first (tests/secp_ecdh_model.py edge_rows: the scalar and curve rules, the
        ladder's edge scalars on G and three of them on each other edge point, coordinates >= p, the
        leading-zero X, the static vector both ways); seeded random rows fill up to 96.  The full cross of
        edge scalars and edge points is run against the reference build by the GPU test itself.
  static  the reference's own vector (crypto/ecies/ecies_test.go:458-485): the two secret keys and the
        shared secret
  unreduced  which coordinate >= p cases the search found ("x+p" always; "y+p" when a curve point with
        y < 2^16 exists)

    python tests/golden/make_secp_ecdh.py
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
import secp_ecdh_model as M  # noqa: E402
from oracle import oracle as O  # noqa: E402

ROWS = 96


def ref_scalar_mul(R, point64: bytes, scalar32: bytes):
    buf = ctypes.create_string_buffer(point64, 64)
    rc = R.secp256k1_ext_scalar_mul(None, buf, ctypes.c_char_p(scalar32))
    return int(rc), buf.raw


def main():
    R = O.ref()
    assert R is not None, "the reference build (make -C oracle ref) is needed"
    cases = M.edge_rows()
    assert len(cases) <= ROWS
    cases += M.random_rows(ROWS - len(cases))
    rows = []
    for tag, point, scalar in cases:
        rc, out = ref_scalar_mul(R, point, scalar)
        k = int.from_bytes(scalar, "big")
        x, y = int.from_bytes(point[:32], "big") % M.P, int.from_bytes(point[32:], "big") % M.P
        if rc == 0:
            assert out == point, "the reference touched its buffer on failure"
            status = M.ST_INVALID_KEY
        else:
            assert rc == 1 and 0 < k < M.N
            status = M.ST_OK if M.on_curve(x, y) else M.ST_INVALID_CURVE
        good = status == M.ST_OK
        shared = out[:32] if good else bytes(32)
        rows.append({"tag": tag, "point": point.hex(), "scalar": scalar.hex(), "ref_rc": rc, "ref_out": out.hex(),
                     "status": status, "out": (out if good else bytes(64)).hex(), "shared": shared.hex(),
                     "keys48": (M.kdf_keys(shared) if good else bytes(48)).hex()})
    with open(os.path.join(HERE, "secp_ecdh.json"), "w") as f:
        json.dump({"source": "secp256k1_ext_scalar_mul (crypto/secp256k1/ext.h) of the reference build, through ctypes; "
                             "keys48 by hashlib",
                   "seed": M.SEED,
                   "static": {"prv1": M.STATIC_PRV1.hex(), "prv2": M.STATIC_PRV2.hex(), "shared": M.STATIC_SHARED.hex()},
                   "unreduced": [t for t, _, _ in M.unreduced_cases()],
                   "rows": rows}, f, indent=1)
        f.write("\n")
    st = [r["status"] for r in rows]
    print("wrote secp_ecdh.json:", len(rows), "rows; statuses", {s: st.count(s) for s in sorted(set(st))},
          "unreduced", [t for t, _, _ in M.unreduced_cases()])


if __name__ == "__main__":
    main()
