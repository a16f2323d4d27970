"""CPU tests of the ecies.Encrypt / Decrypt feature: the Python model (tests/ecies_model.py) against the
published AES vectors and the reference's own handshake packets (tests/golden/ecies_rlpx.json, from
p2p/rlpx_test.go), the committed fixture against a regeneration, and the boundary (header, bindings,
argument checks that precede every HIP call, the mirrors' host-side rules).  No GPU."""
import ctypes
import importlib.util
import os
import re

import pytest

import ecies_model as M
from conftest import GOLDEN, ROOT, golden

E = M.E
NEW = ["gsv_ecies_decrypt_batch", "gsv_ecies_encrypt_batch", "gsv_ecies_decrypt_batch_dev",
       "gsv_ecies_encrypt_batch_dev"]
RLPX_LENS = [194, 322, 327, 97, 377, 383]


# ---------------------------------------------------------------- the model's primitives
def test_fips197_c1():
    w = M.aes128_expand(bytes.fromhex("000102030405060708090a0b0c0d0e0f"))
    assert bytes(w[43]).hex() == "4d2b30c5"  # C.1 round[10].k_sch
    assert M.aes128_encrypt_block(w, bytes.fromhex("00112233445566778899aabbccddeeff")).hex() == \
        "69c4e0d86a7b0430d8cdb78070b4c55a"
    w = M.aes128_expand(bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c"))
    assert bytes(w[43]).hex() == "b6630ca6"  # FIPS-197 A.1
    assert bytes(w[4]).hex() == "a0fafe17"


def test_sp800_38a_f51_ctr_aes128():
    key = bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c")
    iv = bytes.fromhex("f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff")
    pt = bytes.fromhex("6bc1bee22e409f96e93d7e117393172a" "ae2d8a571e03ac9c9eb76fac45af8e51"
                       "30c81c46a35ce411e5fbc1191a0a52ef" "f69f2445df4f9b17ad2b417be66c3710")
    ct = bytes.fromhex("874d6191b620e3261bef6864990db6ce" "9806f66b7970fdff8617187bb9fffdff"
                       "5ae4df3edbd5d35e5b4f09020db03eab" "1e031dda2fbe03d1792170a0f3009cee")
    assert M.aes128_ctr(key, iv, pt) == ct and M.aes128_ctr(key, iv, ct) == pt
    assert M.aes128_ctr(key, iv, pt[:17]) == ct[:17]


def test_ctr_counter_carries_through_all_128_bits():
    key = bytes(range(16))
    w = M.aes128_expand(key)
    ks = M.aes128_ctr(key, b"\xff" * 16, bytes(48))
    assert ks[:16] == M.aes128_encrypt_block(w, b"\xff" * 16)
    assert ks[16:32] == M.aes128_encrypt_block(w, bytes(16))  # wrapped
    assert ks[32:] == M.aes128_encrypt_block(w, bytes(15) + b"\x01")
    ks = M.aes128_ctr(key, bytes(8) + b"\xff" * 8, bytes(32))
    assert ks[16:] == M.aes128_encrypt_block(w, bytes(7) + b"\x01" + bytes(8))


# ---------------------------------------------------------------- the reference's packets
def _packets():
    rl = golden("ecies_rlpx.json")
    out = []
    for p in rl["packets"]:
        raw = bytes.fromhex(p["packet"])
        s2, c = (raw[:2], raw[2:]) if p["eip8"] else (b"", raw)
        out.append((p["name"], c, bytes.fromhex(rl[p["key"]]), s2))
    return rl, out


def test_rlpx_packets_open(oracle):
    rl, pk = _packets()
    assert [n for n, _, _, _ in pk] == ["auth1", "auth2", "auth3", "ack1", "ack2", "ack3"]
    assert [p["key"] for p in rl["packets"]] == ["keyB"] * 3 + ["keyA"] * 3
    msgs = []
    for (name, c, key, s2), want in zip(pk, RLPX_LENS):
        if s2:
            assert int.from_bytes(s2, "big") == len(c), name  # the EIP-8 size prefix
        st, m = M.decrypt(c, key, s2)
        assert st == M.ST_OK and len(m) == want == len(c) - M.OVERHEAD, name
        assert M.decrypt(c, key, b"" if s2 else b"\x00\x00")[0] == M.ST_INVALID_MESSAGE, name
        msgs.append(m)
    pub = {k: E.pt64(E.ec_mul(int(rl[k], 16), E.G)) for k in ("keyA", "keyB", "ephA", "ephB")}
    nonce_a, nonce_b = bytes.fromhex(rl["nonceA"]), bytes.fromhex(rl["nonceB"])
    # authMsgV4 (p2p/rlpx.go:396-409): signature || Keccak256(ephemeral pubkey) || pubkey || nonce || 00
    assert msgs[0] == bytes.fromhex(rl["authSignature"]) + oracle.keccak256(pub["ephA"]) + pub["keyA"] + nonce_a + b"\0"
    # authRespV4 (p2p/rlpx.go:411-418): ephemeral pubkey || nonce || 00
    assert msgs[3] == pub["ephB"] + nonce_b + b"\0"
    assert len(msgs[0]) == 65 + 32 + 64 + 32 + 1 and len(msgs[3]) == 64 + 32 + 1
    assert len(pk[0][1]) == 307


# ---------------------------------------------------------------- the fixture
def test_fixture_is_the_models():
    spec = importlib.util.spec_from_file_location("make_ecies", os.path.join(GOLDEN, "make_ecies.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.fixture() == golden("ecies.json")
    assert os.path.getsize(os.path.join(GOLDEN, "ecies.json")) < 200_000


def test_fixture_covers_what_the_issue_lists():
    fx = golden("ecies.json")
    good, bad = fx["good"], fx["bad"]
    lens = [len(r["msg"]) // 2 for r in good if r["tag"] == "len"]
    assert lens == list(M.MSG_LENS) == [0, 1, 15, 16, 17, 38, 39, 40, 47, 48, 49, 97, 102, 103, 104, 194, 1000]
    assert {len(r["s2"]) // 2 for r in good} == {0, 2, 7, 64}
    carry = [r for r in good if r["tag"] == "carry"]
    assert {r["iv"] for r in carry} == {"ff" * 16, "00" * 12 + "ff" * 4, "00" * 8 + "ff" * 8}
    assert all(len(r["msg"]) // 2 >= 33 for r in carry)
    for r in good:
        want = M.ST_INVALID_MESSAGE if not r["msg"] else M.ST_OK
        assert r["status"] == want
        assert len(r["ct"]) // 2 == M.OVERHEAD + len(r["msg"]) // 2
        if want != M.ST_OK:
            assert not any(bytes.fromhex(r["ct"]))
    # every numbered failure, and the listed ones by tag
    assert {r["tag"].split()[0] for r in bad} == {str(k) for k in range(1, 11)}
    tags = {r["tag"] for r in bad}
    assert {"9 first tag byte", "9 last tag byte", "9 ciphertext bit", "9 wrong s2", "3 len 97", "8 len 98",
            "8 len 112", "10 len 113"} <= tags
    by = {r["tag"]: r for r in bad}
    assert [len(by[t]["ct"]) // 2 for t in ("3 len 97", "8 len 98", "8 len 112", "10 len 113")] == [97, 98, 112, 113]
    assert by["10 len 113"]["status"] == 0 and by["10 len 113"]["msg"] == ""
    assert by["6 off curve, bad key"]["status"] == M.ST_INVALID_CURVE  # the curve before the key
    assert by["7 key 0, len 98"]["status"] == M.ST_INVALID_KEY         # the key before the short em
    assert by["2 first byte 05, one byte long"]["status"] == M.ST_INVALID_PUBKEY  # whatever the length
    for r in bad:
        if r["status"] != 0:
            assert r["msg"] == ""


def test_model_round_trip_and_encrypt_rules():
    fx = golden("ecies.json")
    r = fx["good"][5]
    msg, pub, eph, iv, s2 = (bytes.fromhex(r[k]) for k in ("msg", "pub", "eph", "iv", "s2"))
    assert M.encrypt(msg, pub, eph, iv, s2) == (0, bytes.fromhex(r["ct"]))
    assert M.encrypt(msg, pub, bytes(32), iv, s2) == (M.ST_INVALID_KEY, bytes(M.OVERHEAD + len(msg)))
    assert M.encrypt(msg, pub, E.be32(E.N), iv, s2)[0] == M.ST_INVALID_KEY
    off = E.be32(E.GX) + E.be32(E.GY + 1)
    assert M.encrypt(msg, off, eph, iv, s2)[0] == M.ST_INVALID_CURVE
    assert M.encrypt(msg, off, bytes(32), iv, s2)[0] == M.ST_INVALID_KEY  # the key rule first
    assert M.encrypt(b"", pub, eph, iv, s2) == (M.ST_INVALID_MESSAGE, bytes(M.OVERHEAD))
    assert M.encrypt(b"", off, eph, iv, s2)[0] == M.ST_INVALID_CURVE


# ---------------------------------------------------------------- the boundary
def test_boundary_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, "include", "gsv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from gsv import _lib
    L = _lib.load()
    bound = {n: a for n, _, a in _lib.SIGNATURES}
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, code), s
        assert hasattr(L, s) and s in bound, s
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % s, code).group(1)
        assert len(bound[s]) == decl.count(",") + 1, s
    assert hasattr(L, "gsv_ecies_work_bytes") and "gsv_ecies_work_bytes" in bound
    assert int(re.search(r"#define GSV_ST_INVALID_MESSAGE (\d+)", txt).group(1)) == _lib.ST_INVALID_MESSAGE == 14
    assert int(re.search(r"#define GSV_ECIES_OVERHEAD (\d+)", txt).group(1)) == _lib.ECIES_OVERHEAD == M.OVERHEAD == 113
    assert int(re.search(r"#define GSV_K_ECIES (\d+)", txt).group(1)) == _lib.K_ECIES
    assert int(re.search(r"#define GSV_K_END (\d+)", txt).group(1)) == _lib.K_ECIES + 1
    assert _lib.STATUS_STRINGS[_lib.ST_INVALID_MESSAGE] == "ecies: invalid message"
    assert (M.ST_INVALID_PUBKEY, M.ST_INVALID_KEY, M.ST_INVALID_CURVE) == \
        (_lib.ST_INVALID_PUBKEY, _lib.ST_INVALID_KEY, _lib.ST_INVALID_CURVE)
    # the work area: 48 (Ke || Km) + R + the status bytes the launches hand each other, per item
    assert L.gsv_ecies_work_bytes(0, 0) == 0 and L.gsv_ecies_work_bytes(1000, 0) == 113_000
    assert L.gsv_ecies_work_bytes(1000, 1) == 115_000


def test_arguments_are_checked_without_a_device():
    """the checks precede every HIP call: a NULL context; with a context that is never dereferenced, a NULL
    required pointer, n past 2^32 - 1, a descending table, an item of 2^32 bytes"""
    from gsv import _lib
    L = _lib.load()
    EA, EL = _lib.E_INVALID_ARG, _lib.E_TOO_LARGE
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    off = (ctypes.c_uint64 * 2)(0, 120)
    po = ctypes.cast(off, ctypes.c_void_p)
    dec = [p, po, p, None, None, 1, p, p, p]
    enc = [p, po, p, p, p, None, None, 1, p, p]
    assert L.gsv_ecies_decrypt_batch(None, *dec) == EA and L.gsv_ecies_encrypt_batch(None, *enc) == EA
    assert L.gsv_ecies_decrypt_batch_dev(None, *dec, p, None) == EA
    assert L.gsv_ecies_encrypt_batch_dev(None, *enc, p, None) == EA
    fake = p
    for k in (0, 1, 2, 6, 7, 8):
        a = list(dec)
        a[k] = None
        assert L.gsv_ecies_decrypt_batch(fake, *a) == EA, k
        assert L.gsv_ecies_decrypt_batch_dev(fake, *a, p, None) == EA, k
    assert L.gsv_ecies_decrypt_batch_dev(fake, *dec, None, None) == EA  # no work area
    for k in (0, 1, 2, 3, 4, 8, 9):
        a = list(enc)
        a[k] = None
        assert L.gsv_ecies_encrypt_batch(fake, *a) == EA, k
        assert L.gsv_ecies_encrypt_batch_dev(fake, *a, p, None) == EA, k
    assert L.gsv_ecies_encrypt_batch_dev(fake, *enc, None, None) == EA
    big = list(dec)
    big[5] = 1 << 32
    assert L.gsv_ecies_decrypt_batch(fake, *big) == EA and L.gsv_ecies_decrypt_batch_dev(fake, *big, p, None) == EA
    down = (ctypes.c_uint64 * 2)(8, 0)
    huge = (ctypes.c_uint64 * 2)(0, 1 << 32)
    for tab, want in ((down, EA), (huge, EL)):
        pt = ctypes.cast(tab, ctypes.c_void_p)
        assert L.gsv_ecies_decrypt_batch(fake, p, pt, p, None, None, 1, p, p, p) == want
        assert L.gsv_ecies_encrypt_batch(fake, p, pt, p, p, p, None, None, 1, p, p) == want
        assert L.gsv_ecies_decrypt_batch(fake, p, po, p, p, pt, 1, p, p, p) == want  # the s2 table
        assert L.gsv_ecies_encrypt_batch(fake, p, po, p, p, p, p, pt, 1, p, p) == want
    # n = 0 is success and touches nothing
    assert L.gsv_ecies_decrypt_batch(fake, None, None, None, None, None, 0, None, None, None) == 0
    assert L.gsv_ecies_encrypt_batch(fake, None, None, None, None, None, None, None, 0, None, None) == 0
    assert L.gsv_ecies_decrypt_batch_dev(fake, None, None, None, None, None, 0, None, None, None, None, None) == 0
    assert L.gsv_ecies_encrypt_batch_dev(fake, None, None, None, None, None, None, None, 0, None, None, None, None) == 0


def test_python_mirrors_host_side_rules():
    from gsv import ecies
    with pytest.raises(NotImplementedError):
        ecies.Decrypt(1, b"\x04" + bytes(112), s1=b"x")
    with pytest.raises(NotImplementedError):
        ecies.Encrypt(os.urandom, E.pt64(E.G), b"m", s1=b"x")
    assert ecies.ErrInvalidMessage.__doc__ == "ecies: invalid message"
    assert ecies.ErrInvalidPublicKey.__doc__ == "ecies: invalid public key"
    assert issubclass(ecies.ErrInvalidMessage, ValueError) and issubclass(ecies.ErrInvalidPublicKey, ValueError)
    assert "NotImplementedError" in ecies.__doc__ and "is not here" not in ecies.__doc__ and "are not here" not in ecies.__doc__
    assert ecies._N == E.N
