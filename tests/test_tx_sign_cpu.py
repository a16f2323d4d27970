"""CPU side of batched types.SignTx: the model tests/tx_sign_model.py against the recorded rows of
tests/golden/tx_sign.json and the oracle's types.Sender, GSV_TX_SIGN_GROWTH against the model's worst case,
the host-side preparation of the signer's bytes (csrc/txsign_params.h, compiled with g++), and the argument
checks of the C ABI that need no GPU.  The signer here is the oracle's with tests/rfc6979_model.py's nonce
(tests/test_rfc6979_cpu.py ties it to the reference's); where the reference build is present its own
signer is run over the same rows."""
import ctypes
import os
import re

import pytest

import tx_rules_corpus as RC
import tx_rules_model as M
import tx_sign_corpus as C
import tx_sign_model as S
from conftest import ROOT, build_native, golden


@pytest.fixture(scope="module")
def rows():
    return golden("tx_sign.json")["rows"]


def _row(r):
    return bytes.fromhex(r["rlp"]), bytes.fromhex(r["key"]), r["signer"], int(r["chain_id"], 16)


@pytest.fixture(scope="module")
def diff(oracle):
    items = C.differential()
    sign = C.model_signer(oracle)
    return items, [S.sign_tx(b, k, s, c, sign, oracle.keccak256) for b, k, s, c in items]


# ---------------------------------------------------------------- the fixture
def test_model_reproduces_the_fixture(oracle, rows):
    signers = [C.model_signer(oracle)] + ([C.ref_signer(oracle)] if oracle.ref_available() else [])
    assert len(rows) >= 80
    for sign in signers:
        for r in rows:
            st, signed, h = S.sign_tx(*_row(r), sign, oracle.keccak256)
            assert (st, signed.hex(), h.hex()) == (r["status"], r["signed"], r["hash"]), r["label"]
    assert {r["status"] for r in rows} == {S.ST_OK, S.ST_BAD_RLP, S.ST_INVALID_KEY}
    assert {(r["signer"], int(r["chain_id"], 16)) for r in rows} >= set(C.GROUPS)


def test_fixture_is_what_its_generator_builds(oracle, rows):
    """the inputs are tests/tx_sign_corpus.py's, so a change there cannot leave the file behind"""
    short = {r["label"]: bytes.fromhex(r["rlp"]) for r in rows[:len(C.SHORT_CLASSES)]}
    want = C.fixture_inputs(oracle, short)
    assert [(r["label"],) + _row(r) for r in rows] == want


def test_fixture_holds_the_short_signature_classes(rows):
    lens = [C.sig_lens(bytes.fromhex(r["signed"])) for r in rows if r["status"] == S.ST_OK]
    for name, pred in C.SHORT_CLASSES:
        assert any(pred(rl, sl) for rl, sl in lens), name
    # and the long ones: 32-byte halves whose top bit is set take 33 bytes of RLP
    assert any(rl == 32 for rl, _ in lens) and any(sl == 32 for _, sl in lens)


def test_signed_output_keeps_the_six_fields_and_recovers_the_key(oracle, rows):
    n_ok = 0
    for r in rows:
        if r["status"] != S.ST_OK:
            assert r["signed"] == "" and r["hash"] == "00" * 32
            continue
        blob, key, signer, cid = _row(r)
        a, b = M.decode_txdata(blob), M.decode_txdata(bytes.fromhex(r["signed"]))
        for f in RC.FIELDS[:6]:
            assert a[f] == b[f], (r["label"], f)
        want = oracle.keccak256(oracle.secp_pubkey(key)[1:])[12:]
        # the signature is the key's over the hash that was signed, for every row; and types.Sender under
        # the same signer gives the key's address back wherever it is SignTx's inverse
        assert C.signer_address(oracle, bytes.fromhex(r["signed"]), signer, cid) == want, r["label"]
        st, addr = oracle.tx_sender(bytes.fromhex(r["signed"]), cid, signer)
        if C.sender_is_inverse(signer, cid):
            assert st == 0 and addr == want, r["label"]
        else:
            assert (st, addr) != (0, want), r["label"]
        n_ok += 1
    assert n_ok >= 70


def test_resigning_gives_the_same_output(rows):
    by = {r["label"]: r for r in rows}
    again = [r for r in rows if r["label"].endswith(", signed before")]
    assert len(again) >= 10
    for r in again:
        first = by[r["label"][:-len(", signed before")]]
        assert r["rlp"] != first["rlp"] and r["signed"] == first["signed"] and r["hash"] == first["hash"]


# ---------------------------------------------------------------- the differential set (no GPU: its coverage)
def test_differential_set_covers_the_axes(oracle, diff):
    items, exp = diff
    assert len(items) == 4096 and all(e[0] == S.ST_OK for e in exp)
    assert {(s, c) for _, _, s, c in items} == set(C.GROUPS)
    txs = [M.decode_txdata(b) for b, _, _, _ in items]
    assert {t["nonce"] for t in txs} >= set(C.NONCES)
    for f in ("price", "value"):
        assert {len(C.be(t[f])) for t in txs} == set(range(33)), f
    assert {len(t["data"]) for t in txs} >= set(C.DATA_LENS)
    assert {t["data"] for t in txs if len(t["data"]) == 1} >= {b"\x7f", b"\x80"}
    rcpt = {"20" if t["to"] else "c0" if _nil_as_list(b) else "80" for t, (b, _, _, _) in zip(txs, items)}
    assert rcpt == {"20", "80", "c0"}
    # Keccak block boundaries of both hashed streams
    pre = {len(S.sighash_pre(t, s, c)) for t, (_, _, s, c) in zip(txs, items)}
    out = {len(e[1]) for e in exp}
    assert pre >= set(C.BLOCK_EDGES) and out >= set(C.BLOCK_EDGES), (sorted(pre)[:40], sorted(out)[:40])
    # list headers that grow: a payload below 56 signed to 56 or more, one below 256 to 256 or more
    def payload(b):
        return len(b) - (1 if b[0] < 0xF8 else 1 + b[0] - 0xF7)
    grow = {(payload(b) < 56, payload(e[1]) >= 56, payload(b) < 256, payload(e[1]) >= 256)
            for (b, _, _, _), e in zip(items, exp)}
    assert any(g[0] and g[1] for g in grow) and any(g[2] and g[3] and not g[0] for g in grow)
    # both encodings of V around a byte boundary (chain id 46: 127 is one byte, 128 is 81 80)
    v46 = {M.decode_txdata(e[1])["v"] for (_, _, s, c), e in zip(items, exp) if c == 46}
    assert v46 == {127, 128}
    assert max(M.decode_txdata(e[1])["v"] for (_, _, s, c), e in zip(items, exp) if c == 2 ** 63 - 18) == 2 ** 64


def _nil_as_list(blob):
    """is the fourth item of the transaction the empty list?"""
    s = M.Stream(blob)
    s.List()
    M.decode_uint(s), M.decode_bigint(s), M.decode_uint(s)
    return s.data[s.rpos] == 0xC0


# ---------------------------------------------------------------- GSV_TX_SIGN_GROWTH
def _growth_macro():
    txt = open(os.path.join(ROOT, "include", "gsv.h")).read()
    m = re.search(r"#define GSV_TX_SIGN_GROWTH\(chain_id_len\) \(\(size_t\)\(chain_id_len\) \+ (\d+)\)", txt)
    return lambda n: n + int(m.group(1))


def test_growth_bounds_the_models_worst_case(oracle, diff):
    from gsv import _lib
    G = _growth_macro()
    top = lambda msg, key: b"\xff" * 64 + b"\x01"  # R and S of 33 bytes of RLP each
    minimal = S.unsigned_tx(0, 0, 0, None, 0, b"")
    assert len(minimal) == 10
    for nbytes in range(0, 65):
        cid = (1 << (8 * nbytes)) - 1 if nbytes else 0  # the largest chain id of that many bytes
        assert G(nbytes) == _lib.tx_sign_growth(nbytes) == S.growth(nbytes)
        for blob in (minimal, S.unsigned_tx(1, 1, 1, C.TO, 1, bytes(30)), S.unsigned_tx(1, 1, 1, C.TO, 1, bytes(230))):
            st, signed, _ = S.sign_tx(blob, b"\x01".rjust(32, b"\0"), M.SIGNER_EIP155, cid, top, oracle.keccak256)
            assert st == S.ST_OK and len(signed) <= len(blob) + G(nbytes), nbytes
    # the bound is reached: the minimal input under a 64-byte chain id
    st, signed, _ = S.sign_tx(minimal, b"\x01".rjust(32, b"\0"), M.SIGNER_EIP155, (1 << 512) - 1, top, oracle.keccak256)
    assert len(signed) == len(minimal) + G(64) == 141
    # and holds over the whole differential set and the fixture
    items, exp = diff
    for (b, _, s, c), e in zip(items, exp):
        assert len(e[1]) <= len(b) + G(len(C.be(c)))


def test_work_area_and_ids_are_declared_and_bound():
    from gsv import _lib
    L = _lib.load()
    txt = open(os.path.join(ROOT, "include", "gsv.h")).read()
    assert L.gsv_tx_sign_work_bytes(0) == 0 and L.gsv_tx_sign_work_bytes(1000) == 114_000
    assert int(re.search(r"#define GSV_K_TX_SIGHASH (\d+)", txt).group(1)) == _lib.K_TX_SIGHASH
    assert int(re.search(r"#define GSV_K_TX_SEAL (\d+)", txt).group(1)) == _lib.K_TX_SEAL
    assert int(re.search(r"#define GSV_K_LIMIT (\d+)", txt).group(1)) == _lib.K_TX_SEAL + 1
    assert int(re.search(r"#define GSV_ABI_VERSION (\d+)", txt).group(1)) == 2


# ---------------------------------------------------------------- the signer's bytes, prepared on the host
def test_host_prepared_suffix_and_v_items(tmp_path):
    lib = build_native("tx_sign_params_host.cpp", tmp_path / "tx_sign_params_host.so")
    buf = ctypes.create_string_buffer(80)
    for cid in C.CHAIN_IDS + (127, 128, 2 ** 512 - 1, (2 ** 512 - 1) // 2 - 17):
        raw = C.be(cid)
        for lead in (b"", b"\0\0"):  # leading zero bytes are ignored
            if len(lead + raw) > 64:
                continue
            for eip155 in (0, 1):
                n = lib.txs_suffix(lead + raw, len(lead + raw), eip155, buf)
                assert buf.raw[:n] == ((M.enc_uint(cid) + b"\x80\x80") if eip155 else b""), (cid, eip155)
                for recid in range(4):
                    n = lib.txs_v_item(lead + raw, len(lead + raw), eip155, recid, buf)
                    sig = bytes(64) + bytes([recid])
                    v = S.sig_values(sig, M.SIGNER_EIP155 if eip155 else M.SIGNER_HOMESTEAD, cid)[2]
                    assert buf.raw[:n] == M.enc_uint(v), (cid, eip155, recid)
                    assert n <= len(raw) + 3


def test_host_code_under_sanitizers(tmp_path):
    """the same host code and the staging layout as a stand-alone program with ASan + UBSan (a plain build
    where the compiler links neither), run as a child process: tests/native/tx_sign_params_main.cpp"""
    import subprocess
    src = os.path.join(ROOT, "tests", "native", "tx_sign_params_main.cpp")
    exe = tmp_path / "tx_sign_params_main"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-o", str(exe), src]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ---------------------------------------------------------------- argument errors, no GPU
def test_arguments_are_checked_without_a_device():
    """GSV_E_INVALID_ARG before any HIP call: a NULL context; with a context that is never dereferenced,
    a chain id of 65 bytes, a NULL chain id with a length, an unknown signer kind, a NULL required pointer"""
    from gsv import _lib
    L = _lib.load()
    EA = _lib.E_INVALID_ARG
    buf = ctypes.create_string_buffer(512)
    p = ctypes.cast(buf, ctypes.c_void_p)
    fake = p
    off = (ctypes.c_uint64 * 2)(0, 10)
    po = ctypes.cast(off, ctypes.c_void_p)

    def host(ctx=fake, cid=p, cidlen=1, kind=0, n=1, rlp=p, offs=po, key=p, out=p, olen=p, h=p, st=p):
        return L.gsv_tx_sign_batch(ctx, rlp, offs, n, key, cid, cidlen, kind, out, olen, h, st)

    def dev(ctx=fake, cid=p, cidlen=1, kind=0, n=1, rlp=p, offs=po, key=p, out=p, olen=p, h=p, st=p, work=p):
        return L.gsv_tx_sign_batch_dev(ctx, rlp, offs, n, key, cid, cidlen, kind, out, olen, h, st, work, None)

    for f in (host, dev):
        assert f(ctx=None) == EA
        assert f(ctx=None, n=0) == EA
        assert f(cidlen=65) == EA and f(cidlen=65, n=0) == EA
        assert f(cid=None, cidlen=1) == EA and f(cid=None, cidlen=1, n=0) == EA
        for kind in (-1, 3, 255):
            assert f(kind=kind) == EA and f(kind=kind, n=0) == EA
        for name in ("offs", "key", "out", "olen", "st"):
            assert f(**{name: None}) == EA, name
        assert f(n=1 << 32) == EA
        # n = 0 is success and touches nothing; a chain id of 0 may come as (NULL, 0)
        assert f(n=0, rlp=None, offs=None, key=None, out=None, olen=None, h=None, st=None, cid=None, cidlen=0) == 0
    assert dev(work=None) == EA and dev(rlp=None) == EA
    down = (ctypes.c_uint64 * 2)(8, 0)
    assert host(offs=ctypes.cast(down, ctypes.c_void_p)) == EA  # the host form checks the table
    misaligned = ctypes.c_void_p(p.value + 1)
    assert dev(work=misaligned) == EA and dev(h=misaligned) == EA and dev(olen=misaligned) == EA


def test_python_mirror_checks_before_any_call():
    import gsv
    from gsv import _lib, types
    c = gsv.Context.__new__(gsv.Context)
    c._h, c.device, c._streams = None, 0, []
    with pytest.raises(ValueError):
        c.tx_sign_batch([b"\xc0"], bytes(32), 1, 3)
    with pytest.raises(ValueError):
        c.tx_sign_batch([b"\xc0"], bytes(32), 1 << 512, _lib.SIGNER_EIP155)
    with pytest.raises(ValueError):
        c.tx_sign_batch([b"\xc0", b"\xc0"], bytes(32), 1, _lib.SIGNER_EIP155)  # one key for two transactions
    with pytest.raises(types.ErrInvalidKey):
        types.SignTxBatch([b"\xc0"], types.HomesteadSigner(), [1 << 256], ctx=c)
    assert c.tx_sign_batch([], [], 1, _lib.SIGNER_EIP155)[0] == []
    assert types.EIP155Signer(5) == types.EIP155Signer(5) != types.EIP155Signer(6)
    assert types.EIP155Signer().chain_id == 0 and types.FrontierSigner().kind == _lib.SIGNER_FRONTIER
    from gsv import crypto
    assert types.ErrInvalidKey is crypto.ErrInvalidKey
