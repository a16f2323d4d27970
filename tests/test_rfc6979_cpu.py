"""CPU tests of the signing path's hash side: a host build (tests/native/rfc6979_host.cpp) of
csrc/sha256_dev.cuh and csrc/rfc6979_dev.cuh against hashlib / hmac and tests/rfc6979_model.py, the
generated constants, the model against the reference's own signer, the recorded rows, and the ABI pins
of the four entry points.  The counters past 0 are reached here and nowhere else: no input anyone can
construct makes the signing kernel take its retry."""
import ctypes
import hashlib
import hmac
import os
import random
import re
import subprocess
import sys

import pytest

import rfc6979_model as M
from conftest import ROOT, golden

CSRC = os.path.join(ROOT, "geth-sharding_amd", "csrc")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    from conftest import build_native
    return build_native("rfc6979_host.cpp", tmp_path_factory.mktemp("rfc6979") / "rfc6979_host.so")


def _buf(n=32):
    return ctypes.create_string_buffer(n)


# ---------------------------------------------------------------- SHA-256 compression
def test_compression_against_hashlib(lib):
    rng = random.Random(1)
    # one block up to 55 bytes, two from 56 on (55 / 56 is the padding's edge), 64 and 119 / 120 the next
    for n in [0, 1, 3, 31, 32, 33, 54, 55, 56, 57, 63, 64, 65, 97, 118, 119, 120, 127, 128, 200]:
        for _ in range(4):
            m = bytes(rng.getrandbits(8) for _ in range(n))
            out = _buf()
            lib.t_sha256(out, m, ctypes.c_size_t(n))
            assert out.raw == hashlib.sha256(m).digest(), n
    for m in (b"\x00" * 64, b"\xff" * 64, b"\xff" * 55, b"\x80" * 56):
        out = _buf()
        lib.t_sha256(out, m, ctypes.c_size_t(len(m)))
        assert out.raw == hashlib.sha256(m).digest()


# ---------------------------------------------------------------- the three HMAC shapes
def _keys_and_values(rng, count):
    rows = [(bytes(32), b"\x01" * 32), (b"\xff" * 32, b"\xff" * 32), (b"\x36" * 32, bytes(32)),
            (b"\x5c" * 32, b"\x80" * 32)]
    rows += [(rng.getrandbits(256).to_bytes(32, "big"), rng.getrandbits(256).to_bytes(32, "big"))
             for _ in range(count)]
    return rows


def test_hmac_shapes_against_hmac(lib):
    rng = random.Random(2)
    for key, v in _keys_and_values(rng, 64):
        out = _buf()
        lib.t_hmac32(out, key, v)
        assert out.raw == hmac.new(key, v, hashlib.sha256).digest()
        for tag in (0, 1, 0x80, 0xff):
            lib.t_hmac33(out, key, v, tag)
            assert out.raw == hmac.new(key, v + bytes([tag]), hashlib.sha256).digest()
            a, b = rng.getrandbits(256).to_bytes(32, "big"), rng.getrandbits(256).to_bytes(32, "big")
            for a_, b_ in ((a, b), (b"\xff" * 32, bytes(32)), (bytes(32), b"\xff" * 32)):
                lib.t_hmac97(out, key, v, tag, a_, b_)
                assert out.raw == hmac.new(key, v + bytes([tag]) + a_ + b_, hashlib.sha256).digest()


# ---------------------------------------------------------------- generated constants
def test_zero_key_midstates_are_the_key_blocks_chaining_values(lib):
    """HMAC0_IPAD / HMAC0_OPAD (sha256_consts.inc) equal what hmac_key computes for the all-zero key, and
    an HMAC made from them equals hmac's: hashlib exposes no chaining value, so they are pinned through
    the function they serve"""
    const, made = _buf(64), _buf(64)
    lib.t_hmac_mid(const, None)
    lib.t_hmac_mid(made, bytes(32))
    assert const.raw == made.raw
    txt = open(os.path.join(CSRC, "sha256_consts.inc")).read()
    words = {nm: [int(x, 16) for x in re.findall(r"0x([0-9a-f]{8})u", body)]
             for nm, body in re.findall(r"uint32_t (\w+)\[\d+\] = \{(.*?)\};", txt, flags=re.S)}
    assert b"".join(w.to_bytes(4, "big") for w in words["HMAC0_IPAD"] + words["HMAC0_OPAD"]) == const.raw
    # the FIPS 180-4 constants: hashlib's digest of the empty message is one compression of the padding
    # block from SHA256_IV with SHA256_K, which t_sha256 runs
    assert len(words["SHA256_K"]) == 64 and len(words["SHA256_IV"]) == 8
    out = _buf()
    lib.t_sha256(out, b"", ctypes.c_size_t(0))
    assert out.raw == hashlib.sha256(b"").digest()


def test_constants_file_is_what_the_generator_writes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_sha256_consts.py"), "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


# ---------------------------------------------------------------- the nonce
def _nonces(lib, pairs, counter):
    out = _buf(32 * len(pairs))
    lib.t_nonce(out, b"".join(k for k, _ in pairs), b"".join(m for _, m in pairs), len(pairs), counter)
    return [out.raw[32 * i:32 * i + 32] for i in range(len(pairs))]


def test_nonce_against_model_counters_0_to_3(lib):
    pairs = M.edge_pairs() + M.random_pairs(256, 3)
    for counter in range(4):
        got = _nonces(lib, pairs, counter)
        for (key, msg), g in zip(pairs, got):
            assert g == M.nonce(key, msg, counter), (key.hex(), msg.hex(), counter)
    # successive counters of one generator differ, and the message enters unreduced: n and 0 differ
    k1 = (1).to_bytes(32, "big")
    assert len({M.nonce(k1, bytes(32), c) for c in range(4)}) == 4
    assert M.nonce(k1, M.N.to_bytes(32, "big")) != M.nonce(k1, bytes(32))


def test_model_is_rfc6979_a_2_5():
    """RFC 6979 A.2.5 (P-256, SHA-256, message "sample") pins the generator's structure: its k is this
    construction's first output for x and h1 = SHA-256("sample") (qlen = hlen = 256, and h1 < q there, so
    bits2octets leaves it as it is)"""
    x = bytes.fromhex("C9AFA9D845BA75166B5C215767B1D6934E50C3DB36E89B127B8A622B120F6721")
    h1 = hashlib.sha256(b"sample").digest()
    assert M.nonce(x, h1).hex().upper() == "A6E3C57DD01ABE90086538398355DD4C3B17AA873382B0F24D6129493D8AAD60"


def test_host_build_under_sanitizers(tmp_path):
    """the same host code as a stand-alone program with ASan + UBSan (a plain build where the compiler
    links neither), run as a child process: tests/native/rfc6979_main.cpp"""
    src = os.path.join(ROOT, "tests", "native", "rfc6979_main.cpp")
    exe = tmp_path / "rfc6979_main"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", str(exe), src]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ---------------------------------------------------------------- the model against the reference
def test_model_signs_as_the_reference_does(oracle):
    R = oracle.ref()
    if R is None:
        pytest.skip("reference build oracle/_ref not present")
    pairs = M.edge_pairs() + M.random_pairs(512 - len(M.edge_pairs()), 4)
    for key, msg in pairs:
        sig = _buf(65)
        assert R.gsvref_sign(sig, msg, key) == 1
        assert oracle.secp_sign(msg, key, M.nonce(key, msg)) == sig.raw, (key.hex(), msg.hex())


def test_golden_rows_are_the_models(oracle):
    """every recorded row is reproduced by the oracle's signer with the model's nonce, and its key by
    the oracle's derivation: the JSON, the model and the oracle agree without the reference build"""
    rows = golden("secp_sign.json")["rows"]
    assert len(rows) == 64
    want_first = [(k.hex(), m.hex()) for k, m in M.edge_pairs()]
    assert [(r["key"], r["msg"]) for r in rows[:len(want_first)]] == want_first
    for r in rows:
        key, msg = bytes.fromhex(r["key"]), bytes.fromhex(r["msg"])
        assert oracle.secp_sign(msg, key, M.nonce(key, msg)).hex() == r["sig"]
        assert oracle.secp_pubkey(key).hex() == r["pub"]
    assert {r["sig"][-2:] for r in rows} == {"00", "01"}


# ---------------------------------------------------------------- ABI pins
def test_invalid_key_status_is_11_in_header_and_binding():
    from gsv import _lib
    txt = open(os.path.join(ROOT, "include", "gsv.h")).read()
    assert int(re.search(r"#define GSV_ST_INVALID_KEY (\d+)", txt).group(1)) == 11 == _lib.ST_INVALID_KEY
    assert int(re.search(r"#define GSV_K_COUNT (\d+)", txt).group(1)) == 12
    assert int(re.search(r"#define GSV_ABI_VERSION (\d+)", txt).group(1)) == 2


def test_sign_entry_points_are_bound_and_check_their_arguments():
    """the four symbols exist with the header's arity, and the null-argument rules answer
    GSV_E_INVALID_ARG before any HIP call (no GPU needed)"""
    from gsv import _lib
    L = _lib.load()
    arity = {n: len(a) for n, _, a in _lib.SIGNATURES}
    assert arity["gsv_ecdsa_sign_batch"] == 6 and arity["gsv_ecdsa_sign_batch_dev"] == 7
    assert arity["gsv_pubkey_create_batch"] == 6 and arity["gsv_pubkey_create_batch_dev"] == 7
    b = ctypes.create_string_buffer(65)
    p = ctypes.cast(b, ctypes.c_void_p)
    E = _lib.E_INVALID_ARG
    assert L.gsv_ecdsa_sign_batch(None, p, p, 1, p, p) == E
    assert L.gsv_ecdsa_sign_batch_dev(None, p, p, 1, p, p, None) == E
    assert L.gsv_pubkey_create_batch(None, p, 1, p, None, p) == E
    assert L.gsv_pubkey_create_batch_dev(None, p, 1, p, None, p, None) == E
    assert L.gsv_ctx_arena_read(None, 0, 1, p) == E


def test_python_sign_checks_lengths_before_any_gpu_call():
    from gsv import crypto
    with pytest.raises(crypto.ErrInvalidMsgLen):
        crypto.Sign(b"\x01" * 31, 1)
    with pytest.raises(crypto.ErrInvalidKey):
        crypto.Sign(b"\x01" * 32, 1 << 256)
    with pytest.raises(crypto.ErrInvalidKey):
        crypto.Sign(b"\x01" * 32, b"\x01" * 33)
    with pytest.raises(crypto.ErrInvalidKey):
        crypto.PubkeyFromSeckey(-1)
    assert crypto._padded_key(1) == bytes(31) + b"\x01" == crypto._padded_key(b"\x01")
