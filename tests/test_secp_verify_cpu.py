"""CPU side of batched ECDSA verification and public-key parsing (gsv_ecdsa_verify_batch,
gsv_pubkey_parse_batch): the Python-integer model (tests/secp_verify_model.py) against the reference's
own vectors (tests/golden/secp_verify.json, from crypto/signature_test.go) and against the
reference-compiled recovery through the identity

    verify(msg, (r, s), key) is true  <=>  the key parses, s <= n/2, and some recid in 0..3 makes
                                          ecrecover(msg, r || s || recid) return the parsed key;

the four C symbols declared, exported and bound; their argument checks, which need no GPU; the length
rules of crypto.VerifySignature; and the host packing of keys into the device layout through a
stand-alone program (tests/native/pubkey_pack_host.cpp, ASan + UBSan when the compiler links them)."""
import ctypes
import os
import random
import re
import subprocess

import pytest

import secp_verify_model as V
from conftest import ROOT, golden

NEW_SYMBOLS = ("gsv_ecdsa_verify_batch", "gsv_ecdsa_verify_batch_dev", "gsv_pubkey_parse_batch",
               "gsv_pubkey_parse_batch_dev")


# ---------------------------------------------------------------- the reference's vectors
def fixture_cases():
    """[(case, key, msg, sig, expect)] of TestVerifySignature and TestVerifySignatureMalleable"""
    g = golden("secp_verify.json")
    sig = bytes.fromhex(g["testsig"])[:-1]  # without the recovery id
    wrong = bytearray(bytes.fromhex(g["testpubkey"]))
    wrong[10] = (wrong[10] + 1) & 0xFF
    names = {"testpubkey": bytes.fromhex(g["testpubkey"]), "testpubkeyc": bytes.fromhex(g["testpubkeyc"]),
             "testmsg": bytes.fromhex(g["testmsg"]), "nil": b"", "sig": sig, "sig+010203": sig + b"\x01\x02\x03",
             "sig-2": sig[:-2], "testpubkey[10]++": bytes(wrong)}
    out = [(c["case"], names[c["key"]], names[c["msg"]], names[c["sig"]], c["expect"]) for c in g["verify_signature"]]
    m = g["malleable"]
    out.append(("malleable", bytes.fromhex(m["key"]), bytes.fromhex(m["msg"]), bytes.fromhex(m["sig"]), m["expect"]))
    return out


def test_model_reproduces_the_reference_vectors():
    cases = fixture_cases()
    assert len(cases) == 9 and sum(e for *_, e in cases) == 2
    for case, key, msg, sig, expect in cases:
        assert V.verify(msg, sig, key) == expect, case
    g = golden("secp_verify.json")
    # TestDecompressPubkey / TestCompressPubkey
    full, comp = bytes.fromhex(g["testpubkey"]), bytes.fromhex(g["testpubkeyc"])
    assert V.reencode(comp) == (full, 1)
    assert V.encode(V.parse_pubkey(full), 2) == comp
    assert V.reencode(b"") == (bytes(65), 0) and V.reencode(comp[:5])[1] == 0 and V.reencode(comp + b"\1\2\3")[1] == 0
    # the malleable vector is the high-s twin of a valid signature
    m = g["malleable"]
    sig = bytes.fromhex(m["sig"])
    twin = sig[:32] + V.be32(V.N - int.from_bytes(sig[32:], "big"))
    assert V.verify(bytes.fromhex(m["msg"]), twin, bytes.fromhex(m["key"]))


def test_model_rejects_every_listed_mutation():
    rng = random.Random(0x7e51)
    d, k = rng.randrange(1, V.N), rng.randrange(1, V.N)
    pt = V.M.ec_mul(d, V.G)
    msg = bytes(rng.getrandbits(8) for _ in range(32))
    sig = V.sign(d, msg, k)
    for form in (4, 2, 6):
        assert V.verify(msg, sig, V.encode(pt, form)), form
    cases = V.rejection_cases(msg, sig, pt)
    assert len(cases) > 30
    for name, m, s, key in cases:
        assert not V.verify(m, s, key), name
    for name, key in V.key_rejections(pt):
        assert V.reencode(key) == (bytes(65), 0), name
    for n in V.BAD_LENGTHS:
        assert any(len(key) == n for _, key in V.key_rejections(pt)), n


def test_craft_verify_reaches_the_chosen_scalars():
    """craft_verify's signature verifies, and its u1, u2 are the ones asked for"""
    rng = random.Random(5)
    for u1, u2 in ((0, 1), (1, 1), (rng.randrange(V.N), rng.randrange(1, V.N)), (5 << 40, V.N - 1)):
        pt, msg, sig = V.point_for(u1, u2, seed=rng.randrange(1, 1 << 64))
        s = int.from_bytes(sig[32:], "big")
        r = int.from_bytes(sig[:32], "big")
        si = pow(s, -1, V.N)
        assert s <= V.HALF_N and int.from_bytes(msg, "big") * si % V.N == u1 and r * si % V.N == u2 % V.N
        assert V.verify(msg, sig, V.encode(pt, 4))
    # the r + n branch: X = P with x_P >= n
    pt = V.first_x_above_n()
    assert V.N < pt[0] < V.P
    r = pt[0] - V.N
    assert V.verify(bytes(32), V.be32(r) + V.be32(r), V.encode(pt, 4))
    assert not V.verify(bytes(32), V.be32(r + 1) + V.be32(r + 1), V.encode(pt, 4))
    assert not V.verify(bytes(32), bytes(64), V.encode(V.M.lift_x(V.N, 0), 4))  # x = n: r = 0


# ---------------------------------------------------------------- the identity with the reference's recovery
def test_model_agrees_with_reference_recovery(oracle):
    if not oracle.ref_available():
        pytest.skip("oracle/_ref is not built")
    R = oracle.ref()

    def recover(msg, sig65):
        pub = ctypes.create_string_buffer(65)
        return pub.raw if R.gsvref_ecrecover(pub, sig65, msg) == 1 else None

    items = V.bulk_items(oracle, 0xb01c, 512)
    verdicts = [V.verify(*it) for it in items]
    assert all(verdicts[0::2]) and not any(verdicts[1::2])
    for i, (msg, sig, key) in enumerate(items):
        assert V.identity_expected(recover, msg, sig, key) == verdicts[i], i
        assert oracle.ecrecover(msg, sig + b"\0")[1] == recover(msg, sig + b"\0"), i


# ---------------------------------------------------------------- the boundary
def test_symbols_declared_exported_bound():
    from gsv import _lib
    txt = open(os.path.join(ROOT, "include", "gsv.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    bound = {n: a for n, _, a in _lib.SIGNATURES}
    for s in NEW_SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % s, txt)
        assert m, s
        assert hasattr(L, s), s
        assert s in bound and len(bound[s]) == m.group(1).count(",") + 1, s
    assert int(re.search(r"#define GSV_ABI_VERSION (\d+)", txt).group(1)) == 2
    assert int(re.search(r"#define GSV_K_COUNT (\d+)", txt).group(1)) == 12


def test_argument_checks_need_no_context():
    from gsv import _lib
    L = _lib.load()
    buf = (ctypes.c_uint8 * 130)()
    off = (ctypes.c_uint64 * 3)(0, 65, 130)
    p = ctypes.cast(buf, ctypes.c_void_p)
    o = ctypes.cast(off, ctypes.c_void_p)
    for n in (0, 2):
        assert L.gsv_ecdsa_verify_batch(None, p, p, p, o, n, p) == _lib.E_INVALID_ARG
        assert L.gsv_ecdsa_verify_batch_dev(None, p, p, p, p, n, p, None) == _lib.E_INVALID_ARG
        assert L.gsv_pubkey_parse_batch(None, p, o, n, p, p) == _lib.E_INVALID_ARG
        assert L.gsv_pubkey_parse_batch_dev(None, p, p, n, p, p, None) == _lib.E_INVALID_ARG


def test_verify_signature_length_rules_need_no_gpu(monkeypatch):
    import gsv
    from gsv import crypto

    def no_context():
        raise AssertionError("the length rules come before any context")

    monkeypatch.setattr(crypto, "default_context", no_context)
    monkeypatch.setattr(gsv, "default_context", no_context)
    g = golden("secp_verify.json")
    key, msg, sig = bytes.fromhex(g["testpubkey"]), bytes.fromhex(g["testmsg"]), bytes.fromhex(g["testsig"])[:-1]
    assert crypto.VerifySignature(b"", msg, sig) is False
    assert crypto.VerifySignature(key, b"", sig) is False
    assert crypto.VerifySignature(key, msg[:31], sig) is False
    assert crypto.VerifySignature(key, msg, b"") is False
    assert crypto.VerifySignature(key, msg, sig + b"\x01\x02\x03") is False
    assert crypto.VerifySignature(key, msg, sig[:-2]) is False
    assert not crypto.VerifySignatureBatch([b"", key, key], [msg, b"", msg], [sig, sig, sig[:-2]]).any()
    for bad in (b"", key[:5], key[:33] + b"\x01\x02\x03", key):
        with pytest.raises(crypto.ErrInvalidPubkey, match="invalid public key"):
            crypto.DecompressPubkey(bad)
    assert issubclass(crypto.ErrInvalidPubkey, ValueError)


# ---------------------------------------------------------------- the host packing
SRC = os.path.join(ROOT, "tests", "native", "pubkey_pack_host.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def test_pubkey_pack_host(tmp_path):
    exe = tmp_path / "pubkey_pack_host"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe), SRC]
    if subprocess.run(base + SAN, capture_output=True).returncode != 0:  # no sanitizer runtime: plain build
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
