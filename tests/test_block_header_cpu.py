"""CPU tests of the block-header path (include/gsv.h, "block headers"): the model (tests/block_header_model.py)
against the two real headers of the reference's tests and against expectations written by hand
(tests/block_header_cases.py), the new ABI values, and the host-only code (csrc/block_header_host.h) as a
stand-alone program under ASan + UBSan."""
import ctypes
import os
import re
import subprocess

import pytest

import block_header_cases as C
import block_header_model as B
from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U256 = (1 << 256) - 1


@pytest.fixture(scope="module")
def fx():
    return golden("block_headers.json")


# ---------------------------------------------------------------- the two reference headers
def test_block1_of_the_reference_decodes_to_its_pinned_fields(fx):
    r = fx["reference"][0]
    blob = bytes.fromhex(r["rlp"])
    assert len(blob) == 508
    h = B.decode_header(blob)
    # core/types/block_test.go:43-51
    assert h["Difficulty"] == 131072 and h["GasLimit"] == 3141592 and h["GasUsed"] == 21000
    assert h["Coinbase"].hex() == "8888f1f195afa192cfee860698584c030f4c9db1"
    assert h["MixDigest"].hex() == "bd4472abb6659ebe3ee06ee4d7b72a00a9f4d001caca51342001075469aff498"
    assert h["Root"].hex() == "ef1552a40b7165c3cd773806b9e0c165b75356e0314bf0706f279c729f51e017"
    assert B.nonce_number(h) == 0xA13A5A8C8F2BB1C4 == r["nonce"] and h["Time"] == 1426516743
    assert B.header_hash(blob).hex() == r["hash"] == "0a5843ac1cb04865017cb35a57b50b07084e5fcee39b5acadade33149f4fff9e"
    assert B.encode_header(h) == blob
    assert B.hash_no_nonce(h).hex() == r["hash_no_nonce"]
    # the seal as the reference's libethash ran it: the recorded verdict, whatever it is
    want = B.ST_INVALID_MIX_DIGEST if bytes.fromhex(r["mix"]) != h["MixDigest"] else \
        B.ST_INVALID_POW if int(r["result"], 16) > U256 // h["Difficulty"] else B.ST_OK
    assert r["seal_status"] == want


def test_mainnet_block_3311058_seals_over_the_models_hash_no_nonce(fx):
    """consensus/ethash/algorithm_test.go:698-713: the reference asserts VerifySeal == nil, and libethash over the
    MODEL's HashNoNonce gave the header's own MixDigest: that pins the encoding and HashNoNonce end to end"""
    r = fx["reference"][1]
    blob = bytes.fromhex(r["rlp"])
    h = B.decode_header(blob)
    assert h["Number"] == 3311058 and h["Difficulty"] == 167925187834220 and h["Extra"] == b"www.bw.com"
    assert B.nonce_number(h) == 0xF400CD0006070C49 == r["nonce"]
    assert B.encode_header(h) == blob and B.hash_no_nonce(h).hex() == r["hash_no_nonce"]
    assert bytes.fromhex(r["mix"]) == h["MixDigest"] and int(r["result"], 16) <= U256 // h["Difficulty"]
    assert r["seal_status"] == B.ST_OK
    # the 13-field payload is 42 bytes shorter and both heads are f9 hi lo
    body = B.encode_fields(h, B.FIELDS[:13])
    assert blob[0] == body[0] == 0xF9 and len(body) == len(blob) - 42 and body[3:] == blob[3:-42]


# ---------------------------------------------------------------- the generated chains
@pytest.mark.parametrize("key", ["chain40", "forks", "forks_no_dao"])
def test_generated_chains_pass_the_model(fx, key):
    ch = fx[key]
    cfg = C.config_of(ch["config"])
    blobs = [bytes.fromhex(x) for x in ch["headers"]]
    st, wants = B.verify_headers(cfg, blobs, bytes.fromhex(ch["parent"]), ch["now"])
    assert st == [B.ST_OK] * len(blobs)
    assert wants == ch["difficulty"]
    assert [B.header_hash(b).hex() for b in blobs] == ch["hash"]
    assert [B.hash_no_nonce(B.decode_header(b)).hex() for b in blobs] == ch["hash_no_nonce"]
    # without the parent, or with another one, header 0 has no ancestor and the rest is untouched
    assert B.verify_headers(cfg, blobs, None, ch["now"])[0] == [B.ST_UNKNOWN_ANCESTOR] + [B.ST_OK] * (len(blobs) - 1)
    assert B.verify_headers(cfg, blobs, blobs[3], ch["now"])[0][0] == B.ST_UNKNOWN_ANCESTOR


def test_fork_chain_uses_all_three_rules_and_both_dao_verdicts(fx):
    ch = fx["forks"]
    cfg = C.config_of(ch["config"])
    assert (cfg.homestead, cfg.dao, cfg.eip150, cfg.byzantium) == (3, 5, 7, 9) and cfg.dao_support
    blobs = [bytes.fromhex(x) for x in ch["headers"]]
    assert cfg.eip150_hash == B.header_hash(blobs[6])
    # under the other configuration the pro-fork chain fails in the window, and the other way round
    other = C.config_of(fx["forks_no_dao"]["config"])
    st = B.verify_headers(other, blobs, bytes.fromhex(ch["parent"]), ch["now"])[0]
    assert st[4:14] == [B.ST_BAD_NO_DAO_EXTRA] * 10 and st[:4] == [0] * 4 and st[14:] == [0] * 2
    nb = [bytes.fromhex(x) for x in fx["forks_no_dao"]["headers"]]
    st = B.verify_headers(cfg, nb, bytes.fromhex(ch["parent"]), ch["now"])[0]
    # the window fails pro-fork; behind it header 7 of this chain has another hash than the configured one
    assert st[4:14] == [B.ST_BAD_PRO_DAO_EXTRA] * 10 and st[:4] == [0] * 4
    cfg2 = C.config_of(ch["config"])
    cfg2.dao = None
    assert B.verify_headers(cfg2, nb, bytes.fromhex(ch["parent"]), ch["now"])[0][6] == B.ST_FORK_HASH
    cfg2.eip150_hash = bytes(32)  # a zero hash is not checked (misc/forks.go:37)
    assert B.verify_headers(cfg2, nb, bytes.fromhex(ch["parent"]), ch["now"])[0] == [0] * 16


# ---------------------------------------------------------------- decode, lengths
def test_decode_corpus_against_the_expectations_written_by_hand():
    corpus = C.decode_corpus()
    assert len(corpus) >= 60
    for name, blob, want in corpus:
        assert B.decode_status(blob)[0] == want, name
    assert {w for _, _, w in corpus} == {B.ST_OK, B.ST_BAD_RLP, B.ST_HEADER_TOO_WIDE}


def test_length_sweep_covers_the_block_edges():
    hs = C.length_sweep()
    blobs = [B.encode_header(h) for h in hs]
    lens = {len(b) for b in blobs}
    assert {543, 544, 545, 627, 628, 629} <= lens  # Hash at 4 | 5 permutations; HashNoNonce (42 shorter) too
    for b, h in zip(blobs, hs):
        assert B.decode_status(b) == (B.ST_OK, h)
    # where the payload passes 2^16 the header's list head is four bytes and HashNoNonce's still three
    heads = {(b[0], B.encode_fields(h, B.FIELDS[:13])[0]) for b, h in zip(blobs, hs) if len(b) > 60000}
    assert heads == {(0xF9, 0xF9), (0xFA, 0xF9), (0xFA, 0xFA)}


# ---------------------------------------------------------------- the rules
@pytest.fixture(scope="module")
def anchor():
    parent = B.new_header(Difficulty=1 << 20, Number=7, GasLimit=5000000, Time=1500000000, Extra=b"anchor")
    return parent, B.encode_header(parent), 1500000000 + 100000


def test_each_check_fails_alone_and_pairs_show_the_order(anchor):
    parent, pb, now = anchor
    seen = set()
    for k, (name, over, want) in enumerate(C.rule_cases(parent, now)):
        blobs, at = C.rule_segment(parent, pb, over, 3 * k)
        st, _ = B.verify_headers(C.TEST_CONFIG, blobs, pb, now)
        assert st[0] == B.ST_OK and st[at] == want, (name, st)
        seen.add(want)
    assert seen == {B.ST_OK} | set(range(B.ST_EXTRA_TOO_LONG, B.ST_INVALID_NUMBER + 1))


def test_gas_cases_against_the_expectations_written_by_hand(anchor):
    _, _, now = anchor
    for pg, gl, gu, want in C.gas_cases():
        parent = B.new_header(Difficulty=1 << 20, Number=7, GasLimit=pg, Time=1500000000)
        pb = B.encode_header(parent)
        h = C.child(C.TEST_CONFIG, parent, pb, GasLimit=gl, GasUsed=gu)
        st, _ = B.verify_headers(C.TEST_CONFIG, [B.encode_header(h)], pb, now)
        assert st == [want], (pg, gl, gu)


def test_calc_difficulty_by_hand():
    fr, ho, by = B.Config(), B.Config(homestead=0), B.Config(homestead=0, byzantium=0)
    p = B.new_header(Difficulty=1 << 30, Number=50, Time=1000)
    step = (1 << 30) // 2048
    assert B.calc_difficulty(fr, 1012, p) == (1 << 30) + step and B.calc_difficulty(fr, 1013, p) == (1 << 30) - step
    assert B.calc_difficulty(ho, 1009, p) == (1 << 30) + step and B.calc_difficulty(ho, 1010, p) == 1 << 30
    assert B.calc_difficulty(ho, 1000 + 10 ** 6, p) == (1 << 30) - 99 * step
    assert B.calc_difficulty(by, 1008, p) == (1 << 30) + step and B.calc_difficulty(by, 1009, p) == 1 << 30
    u = dict(p, UncleHash=bytes(32))
    assert B.calc_difficulty(by, 1008, u) == (1 << 30) + 2 * step and B.calc_difficulty(by, 1018, u) == 1 << 30
    low = B.new_header(Difficulty=131072, Number=50, Time=1000)
    assert B.calc_difficulty(fr, 2000, low) == B.calc_difficulty(ho, 2000, low) == B.calc_difficulty(by, 2000, low) == 131072
    # the bomb: 2^(period - 2) from period 2 on, by parent.Number + 1 (Byzantium: delayed by 2,999,999)
    for number, bomb in ((99999, 0), (199998, 0), (199999, 1), (299999, 2)):
        q = dict(low, Number=number)
        assert B.calc_difficulty(ho, 2000, q) == 131072 + bomb == B.calc_difficulty(fr, 2000, q)
    for number, bomb in ((2999999, 0), (3199998, 0), (3199999, 1), (3200000, 1)):
        assert B.calc_difficulty(by, 2000, dict(low, Number=number)) == 131072 + bomb, number
    assert B.calc_difficulty(ho, 2000, dict(low, Number=25699999)) == 131072 + (1 << 255)  # period 257
    assert B.calc_difficulty(ho, 2000, dict(low, Number=25799999)) == 131072 + (1 << 256) > U256
    # a time before the parent's: big.Int.Div floors, so -1 // 10 is -1 and the factor is 2
    assert B.calc_difficulty(ho, 999, p) == (1 << 30) + 2 * step
    # the shared cases reach every branch: all three rules, both signs of the factor, a value past 2^256
    cases = C.difficulty_cases()
    vals = [B.calc_difficulty(cfg, t, p) for cfg, t, p in cases]
    assert len(cases) > 350 and sum(v > U256 for v in vals) >= 8 and min(vals) == 131072


# ---------------------------------------------------------------- the ABI
def test_abi_pins_of_the_block_header_path():
    from gsv import _lib
    txt = open(os.path.join(ROOT, "include", "gsv.h")).read()

    def val(name):
        return int(re.search(r"#define %s (\d+)" % name, txt).group(1))
    names = ["HEADER_TOO_WIDE", "UNKNOWN_ANCESTOR", "EXTRA_TOO_LONG", "FUTURE_BLOCK", "ZERO_BLOCK_TIME",
             "WRONG_DIFFICULTY", "GAS_LIMIT_CAP", "GAS_USED", "GAS_LIMIT_BOUNDS", "INVALID_NUMBER", "BAD_PRO_DAO_EXTRA",
             "BAD_NO_DAO_EXTRA", "FORK_HASH"]
    for k, name in enumerate(names):
        assert val("GSV_ST_" + name) == getattr(_lib, "ST_" + name) == getattr(B, "ST_" + name) == 20 + k
        assert getattr(_lib, "ST_" + name) in _lib.STATUS_STRINGS
    assert val("GSV_ST_BAD_RLP") == B.ST_BAD_RLP == 8 and val("GSV_ST_NONCE_NOT_FOUND") == 19
    assert val("GSV_K_PEAK") == _lib.K_PEAK == 23  # pinned: the new ids are behind it
    assert val("GSV_K_BLOCK_HEADER") == _lib.K_BLOCK_HEADER == 23
    assert val("GSV_K_BLOCK_RULES") == _lib.K_BLOCK_RULES == 24
    assert val("GSV_K_BLOCK_MERGE") == _lib.K_BLOCK_MERGE == 25
    assert val("GSV_K_SUMMIT") == _lib.K_SUMMIT == 26
    assert val("GSV_ABI_VERSION") == 2
    S = _lib.ChainConfigStruct
    assert ctypes.sizeof(S) == 72
    assert [getattr(S, f).offset for f in ("homestead_block", "dao_fork_block", "eip150_block", "byzantium_block",
                                           "has_homestead", "has_dao_fork", "has_eip150", "has_byzantium",
                                           "dao_fork_support", "reserved", "eip150_hash")] == \
        [0, 8, 16, 24, 32, 33, 34, 35, 36, 37, 40]
    assert re.search(r"uint8_t eip150_hash\[32\];", txt) and re.search(r"uint8_t reserved\[3\];", txt)


def test_params_carry_the_references_values():
    from gsv import params as P
    m = P.MainnetChainConfig  # params/config.go:33-45
    assert (m.HomesteadBlock, m.DAOForkBlock, m.DAOForkSupport, m.EIP150Block, m.ByzantiumBlock) == \
        (1150000, 1920000, True, 2463000, 4370000)
    assert m.EIP150Hash.hex() == "2086799aeebeae135c246c65021c82b4e15a2c451340993aacfd2751886514f0"
    t = P.TestnetChainConfig  # :48-60
    assert (t.HomesteadBlock, t.DAOForkBlock, t.EIP150Block, t.ByzantiumBlock) == (0, None, 0, 1700000)
    r = P.RinkebyChainConfig  # :63-78
    assert (r.HomesteadBlock, r.DAOForkBlock, r.EIP150Block, r.ByzantiumBlock) == (1, None, 2, 1035301)
    for c in (P.AllEthashProtocolChanges, P.TestChainConfig):  # :85, :94
        assert (c.HomesteadBlock, c.DAOForkBlock, c.DAOForkSupport, c.EIP150Block, c.ByzantiumBlock) == \
            (0, None, False, 0, 0) and c.EIP150Hash == bytes(32)
    assert P.AllEthashProtocolChanges.ChainId == 1337 and P.TestChainConfig.ChainId == 1
    assert P.DAOForkBlockExtra == b"dao-hard-fork" == B.DAO_EXTRA and P.DAOForkExtraRange == 10
    st = m.as_struct()
    assert (st.homestead_block, st.has_homestead, st.dao_fork_block, st.has_dao_fork, st.dao_fork_support) == \
        (1150000, 1, 1920000, 1, 1)
    assert bytes(st.eip150_hash) == m.EIP150Hash and bytes(st.reserved) == bytes(3)
    st = t.as_struct()
    assert (st.has_dao_fork, st.dao_fork_block, st.has_homestead, st.homestead_block) == (0, 0, 1, 0)
    assert m.IsHomestead(1150000) and not m.IsHomestead(1149999) and not P.ChainConfig().IsByzantium(10 ** 9)


def test_entry_points_check_their_arguments_without_a_device():
    from gsv import _lib
    L = _lib.load()
    E = _lib.E_INVALID_ARG
    assert L.gsv_block_header_work_bytes(0) == 156 and L.gsv_block_header_work_bytes(2048) == 156 * 2049
    assert L.gsv_block_header_hash_batch(None, None, None, 1, None, None, None) == E
    assert L.gsv_calc_difficulty_batch(None, None, None, None, None, 1, None, None) == E
    assert L.gsv_ethash_verify_headers_batch(None, None, None, None, 1, None, 0, None, 0, 0, None, None, None) == E
    assert L.gsv_block_header_rules_dev(None, None, None, None, 1, None, 0, 0, None, None, None, None, None, None, None,
                                        None, None, None, None) == E
    assert L.gsv_block_header_merge_dev(None, None, None, None, None, 1, None, None) == E


# ---------------------------------------------------------------- host code under sanitizers
def test_host_code_as_a_program_under_sanitizers(tmp_path):
    """tests/native/block_header_host_main.cpp (record layout, configuration, compaction) with ASan + UBSan (a plain
    build where the compiler links neither), run as a child process"""
    src = os.path.join(ROOT, "tests", "native", "block_header_host_main.cpp")
    exe = tmp_path / "block_header_host_main"
    base = ["g++", "-O2", "-g", "-std=c++17", "-Wall", "-o", str(exe), src]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
