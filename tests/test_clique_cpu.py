"""CPU tests of the clique path (include/gsv.h, "clique"): the model (tests/clique_model.py) against the reference's
TestVoting scenarios, the hand-written rule cases (tests/clique_cases.py) and hand-written expectations for a
64-header chain and its mutations; the host fold of the library (csrc/clique_host.h behind gsv_clique_fold, no GPU
involved) against the model on all of those and on 200 seeded random vote chains; the lifetime of a snapshot handle;
the host-only code as a stand-alone program under ASan + UBSan; the new ABI values."""
import ctypes
import functools
import os
import random
import re
import subprocess

import numpy as np
import pytest

import block_header_model as B
import clique_cases as C
import clique_model as M
from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return golden("clique.json")


@functools.lru_cache(maxsize=None)
def _voting_blobs(i):
    return M.voting_headers(golden("clique.json")["voting"][i])


def _addr(name):
    return M.address(M.key_of(name))


# ---------------------------------------------------------------- the model
def test_accounts_of_the_fixture_are_the_models(fx):
    for name, a in fx["accounts"].items():
        assert M.key_of(name).hex() == a["key"] and _addr(name).hex() == a["address"]


def test_sighash_is_the_hash_of_the_header_without_its_seal():
    h = M.real_header(Extra=b"v" * 32 + b"s" * 65, Number=3)
    g = dict(h, Extra=b"v" * 32)
    assert M.sig_hash(h) == B.keccak256(B.encode_header(g)) != B.keccak256(B.encode_header(h))
    signed = M.sign(h, M.key_of("A"))
    assert signed["Extra"][:32] == h["Extra"][:32] and M.sig_hash(signed) == M.sig_hash(h)
    assert M.ecrecover(signed) == (M.ST_OK, _addr("A"))
    assert M.ecrecover(dict(h, Extra=bytes(64))) == (M.ST_MISSING_SIGNATURE, None)
    bad = dict(signed, Extra=signed["Extra"][:-1] + b"\x04")
    assert M.ecrecover(bad) == (M.ST_INVALID_RECID, None)
    zero_r = dict(signed, Extra=signed["Extra"][:-65] + bytes(32) + signed["Extra"][-33:])
    assert M.ecrecover(zero_r) == (M.ST_RECOVER_FAILED, None)


def test_model_reproduces_every_testvoting_result(fx):
    """snapshot_test.go:331-405 over headers built as that test builds them (a nil Difficulty encodes as 80)"""
    assert len(fx["voting"]) == 20
    for i, scn in enumerate(fx["voting"]):
        blobs = _voting_blobs(i)
        snap = M.Snapshot([_addr(n) for n in scn["signers"]], 0, bytes(32))
        cfg = M.CliqueConfig(15, scn["epoch"])
        st, s, applied, _ = M.verify_headers(B.Config(), cfg, blobs, snap, None, 1 << 40)
        assert applied == len(blobs), (i, st)
        assert s.signers() == sorted(_addr(n) for n in scn["results"]), i
        assert s.Number == len(blobs) and s.Hash == B.header_hash(blobs[-1])


def test_voting_headers_encode_a_nil_difficulty_as_80(fx):
    blob = _voting_blobs(0)[0]
    h = B.decode_header(blob)
    assert h["Difficulty"] == 0 and h["GasLimit"] == 0 and h["UncleHash"] == bytes(32) and len(h["Extra"]) == 97
    # the five integers behind the bloom: Difficulty 80, Number 01, GasLimit 80, GasUsed 80, Time 80
    at = 3 + 2 * 33 + 21 + 3 * 33 + 3 + 256  # f9 hi lo, two hashes, Coinbase, three hashes, b9 01 00 and the bloom
    assert blob[at:at + 5] == bytes([0x80, 0x01, 0x80, 0x80, 0x80])


def test_rule_cases_match_the_model():
    cfg = M.CliqueConfig(C.PERIOD, C.EPOCH)
    seen = set()
    for c in C.CASES:
        chain, parent, blob, now = C.build(c)
        f = M.facts_of(chain, cfg, [blob], parent, now)[0]
        assert f["static"] == c["expect"], c["name"]
        seen.add(c["expect"])
    assert seen >= set(range(41, 52)) | {M.ST_OK, M.ST_BAD_RLP, M.ST_HEADER_TOO_WIDE, M.ST_FUTURE_BLOCK, M.ST_FORK_HASH,
                                         M.ST_UNKNOWN_ANCESTOR}
    g = C.genesis_alone()
    assert M.facts_of(B.Config(), cfg, [g], None, C.T0)[0]["static"] == M.ST_OK
    assert M.facts_of(B.Config(), cfg, [g], None, C.T0 - 1)[0]["static"] == M.ST_FUTURE_BLOCK


def test_chain_of_the_fixture_is_the_models(fx):
    ch = fx["chain"]
    signers = [_addr(n) for n in ch["signers"]]
    blobs, snaps = M.build_chain(ch["plan"], signers, ch["epoch"], ch["period"], bytes.fromhex(ch["genesis"]))
    assert B.header_hash(blobs[-1]).hex() == ch["last_hash"]
    assert [B.decode_header(b)["Difficulty"] for b in blobs] == ch["difficulties"]
    assert snaps[-1].signers() == sorted(_addr(n) for n in ch["final_signers"])
    assert set(ch["final_signers"]) == {"A", "C", "D", "E", "F"}  # F voted in, B voted out
    st, s, applied, _ = M.verify_headers(B.Config(), M.CliqueConfig(ch["period"], ch["epoch"]), blobs,
                                         M.Snapshot(signers, 0, B.header_hash(bytes.fromhex(ch["genesis"]))),
                                         bytes.fromhex(ch["genesis"]), 1 << 40)
    assert st == [0] * 64 and applied == 64 and s.state() == snaps[-1].state()
    # written by hand from the votes of the plan: F is in with the third of five votes (block 4), B is out with the
    # fourth of six (block 21); a checkpoint carries the list of the snapshot in front of it
    f, b = _addr("F"), _addr("B")
    assert [v.get("voted") for v in ch["plan"][1:4]] == ["F"] * 3 and [v.get("voted") for v in ch["plan"][17:21]] == ["B"] * 4
    assert f not in snaps[2].Signers and f in snaps[3].Signers and len(snaps[3].Signers) == 6
    assert b in snaps[19].Signers and b not in snaps[20].Signers and len(snaps[20].Signers) == 5
    assert [len(B.decode_header(blobs[k])["Extra"]) - 97 for k in (7, 15, 23, 63)] == [120, 120, 100, 100]
    assert snaps[7].Votes == [] and snaps[7].Tally == {}  # the epoch reset
    assert len(snaps[18].Votes) == 2 and snaps[18].Tally == {b: [False, 2]}
    # behind block n the window holds blocks n - limit + 1 .. n: limit is 4 with six signers, 3 with five
    assert sorted(snaps[10].Recents) == [8, 9, 10, 11] and sorted(snaps[40].Recents) == [39, 40, 41]


# ---------------------------------------------------------------- the library's fold against the model
def lib_snapshot(signers, number, hsh):
    from gsv import clique as Q
    return Q.Snapshot(signers, number, hsh)


def lib_state(s):
    return dict(number=s.Number, hash=s.Hash, signers=s.signers(), recents=s.Recents, votes=s.Votes, tally=s.Tally)


def lib_fold(s, period, epoch, facts):
    from gsv import params as P
    rec = np.frombuffer(b"".join(M.record_bytes(f) for f in facts), np.uint8)
    # the fold reads a checkpoint's signer list from the header's bytes at the record's offsets
    items = [bytes(f["extra_off"]) + f["extra"] for f in facts]
    return s.apply(P.CliqueConfig(period, epoch), rec, items)


def test_fold_equals_the_model_on_testvoting(fx):
    for i, scn in enumerate(fx["voting"]):
        blobs = _voting_blobs(i)
        signers = [_addr(n) for n in scn["signers"]]
        cfg = M.CliqueConfig(15, scn["epoch"])
        want_st, want, want_applied, facts = M.verify_headers(B.Config(), cfg, blobs, M.Snapshot(signers), None, 1 << 40)
        s = lib_snapshot(signers, 0, bytes(32))
        st, applied = lib_fold(s, 15, cfg.epoch, facts)
        assert list(st) == want_st and applied == want_applied == len(blobs), i
        assert lib_state(s) == want.state(), i
        assert s.signers() == sorted(_addr(n) for n in scn["results"]), i


def _relink(blobs, k, plan):
    """re-signs the headers behind k over the hashes in front of them"""
    out = list(blobs)
    for j in range(k + 1, len(out)):
        h = B.decode_header(out[j])
        h["ParentHash"] = B.header_hash(out[j - 1])
        out[j] = B.encode_header(M.sign(h, M.key_of(plan[j]["signer"])))
    return out


def _mutations(ch, blobs):
    """name -> (chain, expected statuses, expected applied), the expectations written by hand.  K is header 37 (block
    38), CP header 31 (block 32, a checkpoint).  Behind a mutated header the tail is re-signed over the new hashes
    (but for the broken link and the first outsider), so the fold, not the link, decides there."""
    plan, K, CP = ch["plan"], 37, 31
    OKS = [0] * 64

    def resign(j, key=None, **kw):
        h = B.decode_header(blobs[j])
        h.update(kw)
        return B.encode_header(M.sign(h, M.key_of(key if key is not None else plan[j]["signer"])))

    def with_(j, blob, relink=True):
        out = blobs[:j] + [blob] + blobs[j + 1:]
        return _relink(out, j, plan) if relink else out

    def seal_bytes(j, f):
        h = B.decode_header(blobs[j])
        h["Extra"] = h["Extra"][:-65] + f(h["Extra"][-65:])
        return B.encode_header(h)

    def only(j, st):
        return OKS[:j] + [st] + OKS[j + 1:]

    def sticky(j, st, behind=None):
        return OKS[:j] + [st] + [behind if behind is not None else st] * (63 - j)

    d = B.decode_header(blobs[K])["Difficulty"]
    ext = B.decode_header(blobs[CP])["Extra"]
    U, A = M.ST_UNAUTHORIZED, M.ST_UNKNOWN_ANCESTOR
    return {
        # verifySeal refuses it, apply does not look at the difficulty: the chain goes on
        "wrong-turn difficulty": (with_(K, resign(K, Difficulty=3 - d)), only(K, M.ST_DIFFICULTY), 64),
        "a recent signer again": (with_(K, resign(K, key=plan[K - 1]["signer"])), sticky(K, U), K),
        # the tail still points at the old hash: header K + 1 has no ancestor, the rest carry the sticky error
        "an outsider's key": (with_(K, resign(K, key="Z"), relink=False), OKS[:K] + [U, A] + [U] * (62 - K), K),
        "sig[64] = 4": (with_(K, seal_bytes(K, lambda s: s[:64] + b"\x04")), sticky(K, M.ST_INVALID_RECID), K),
        "r = 0": (with_(K, seal_bytes(K, lambda s: bytes(32) + s[32:])), sticky(K, M.ST_RECOVER_FAILED), K),
        "a wrong checkpoint list": (with_(CP, resign(CP, Extra=ext[:32] + ext[52:72] + ext[32:52] + ext[72:])),
                                    only(CP, M.ST_CHECKPOINT_SIGNERS), 64),
        "a broken link": (with_(K, resign(K, ParentHash=bytes(range(32))), relink=False), sticky(K, A), K),
        "a time too close": (with_(K, resign(K, Time=B.decode_header(blobs[K - 1])["Time"])),
                             only(K, M.ST_INVALID_TIMESTAMP), 64),
        "the sticky error": (with_(K, resign(K, key="Z")), sticky(K, U), K),
        # block 38 calls itself 39 and the hashes link: no ancestor for it (its parent is 37) nor for the 39 behind it
        # (its parent is a 39, too); from 40 on the numbers follow again and the headers carry apply's
        # errInvalidVotingChain
        "a number that jumps": (with_(K, resign(K, Number=K + 2)), OKS[:K] + [A, A] + [M.ST_VOTING_CHAIN] * (62 - K), K),
    }


def test_mutations_of_the_chain_match_hand_written_expectations_and_the_fold(fx):
    ch = fx["chain"]
    signers = [_addr(n) for n in ch["signers"]]
    genesis = bytes.fromhex(ch["genesis"])
    blobs, snaps = M.build_chain(ch["plan"], signers, ch["epoch"], ch["period"], genesis)
    cfg = M.CliqueConfig(ch["period"], ch["epoch"])
    start = M.Snapshot(signers, 0, B.header_hash(genesis))
    for name, (mut, want_st, want_applied) in _mutations(ch, blobs).items():
        st, s, applied, facts = M.verify_headers(B.Config(), cfg, mut, start.copy(), genesis, 1 << 40)
        assert st == want_st, (name, st)
        assert applied == want_applied and s.Number == want_applied, name
        if want_applied < 64:
            assert s.state() == snaps[want_applied - 1].state(), name
        lib = lib_snapshot(signers, 0, start.Hash)
        lst, lapplied = lib_fold(lib, ch["period"], ch["epoch"], facts)
        assert list(lst) == want_st and lapplied == want_applied and lib_state(lib) == s.state(), name
    # apply's own verdict on the jumping number
    mut = _mutations(ch, blobs)["a number that jumps"][0]
    f = M.facts_of(B.Config(), cfg, mut[37:38], mut[36], 1 << 40)[0]
    assert M.apply_one(snaps[36], ch["epoch"], f) == (None, M.ST_VOTING_CHAIN)


def test_a_handle_lives_only_as_long_as_its_snapshot():
    """The handle of a temporary dangles: CPython collects `snap.copy()` as soon as `.handle` is read, and collecting a
    Snapshot frees the C snapshot.  A caller of the C ABI holds the Snapshot while a call runs."""
    import weakref
    from gsv import clique as Q
    freed = []

    class Watched(Q.Snapshot):
        def close(self):
            if getattr(self, "_h", None):
                freed.append(self._h.value)
            super().close()

    s = Q.Snapshot([_addr("A")], 0, bytes(32))
    w = Watched(_handle=_lib_copy(s))
    r = weakref.ref(w)
    h = w.handle.value
    del w
    assert r() is None and freed == [h]          # freed the moment the last reference went
    held = s.copy()
    assert held.signers() == [_addr("A")]        # a held copy stays good
    held.close()
    held.close()                                 # closing twice frees once
    assert s.signers() == [_addr("A")]


def _lib_copy(s):
    from gsv import _lib
    return _lib.load().gsv_clique_snapshot_copy(s.handle)


def _random_chain(rng):
    """facts of a random vote chain with no signatures behind them (the fold reads signers, not seals): 1-7 signers,
    epoch 3 or 8, mostly signers that may sign, votes on insiders and outsiders, and now and then a fault"""
    pool = [bytes([0x10 + k]) * 20 for k in range(10)]
    nsig = rng.randint(1, 7)
    signers = rng.sample(pool, nsig)
    epoch = rng.choice([3, 8])
    model = M.Snapshot(signers, 0, B.keccak256(b"genesis"))
    start = model.copy()
    facts, prev, number = [], model.Hash, 0
    for _ in range(rng.randint(5, 40)):
        number += 1
        limit = len(model.Signers) // 2 + 1
        recent = {s for b, s in model.Recents.items() if b > number - limit}
        may = [s for s in model.signers() if s not in recent]
        signer = rng.choice(may) if may and rng.random() < 0.93 else rng.choice(pool)
        checkpoint = number % epoch == 0
        vote = rng.choice([0, 0, 1, 1, 1, 2]) if rng.random() < 0.8 else 0
        coinbase = rng.choice(pool) if rng.random() < 0.7 else bytes(20)
        # drops are aimed at signers often, so the signer set (and the recents window) shrinks too
        if vote == 0 and model.Signers and rng.random() < 0.6:
            coinbase = rng.choice(model.signers())
        extra = bytes(32) + (b"".join(model.signers()) if checkpoint else b"") + bytes(65)
        if checkpoint and rng.random() < 0.1:
            extra = bytes(32) + bytes(20) + bytes(65)
        f = dict(static=M.ST_OK, decoded=True, number=number, hash=B.keccak256(prev + bytes([number & 255])),
                 parent_hash=prev, signer_status=M.ST_OK, signer=signer, coinbase=coinbase, vote=vote,
                 difficulty=rng.choice([1, 2]), extra=extra, extra_off=rng.randint(0, 5))
        if signer in model.Signers and rng.random() < 0.8:
            f["difficulty"] = 2 if model.inturn(number, signer) else 1
        r = rng.random()
        if r < 0.02:
            f.update(signer_status=rng.choice([M.ST_INVALID_RECID, M.ST_RECOVER_FAILED, M.ST_MISSING_SIGNATURE]),
                     signer=bytes(20))
        elif r < 0.04:
            f.update(static=M.ST_BAD_RLP, decoded=False, number=0, hash=bytes(32), parent_hash=bytes(32))
        elif r < 0.06:
            f["parent_hash"] = B.keccak256(b"elsewhere")
        elif r < 0.08:
            f["number"] = number + 1
        elif r < 0.12:
            f["static"] = rng.choice([M.ST_MIX_DIGEST, M.ST_INVALID_TIMESTAMP, M.ST_FUTURE_BLOCK, M.ST_HEADER_TOO_WIDE])
        elif r < 0.13:
            f.update(number=0)  # a genesis header in the middle: never applied
        facts.append(f)
        if f["number"] == 0:
            number -= 1  # nothing is applied: the next header stands on the same parent
            continue
        nxt, err = M.apply_one(model, epoch, f)
        if err == M.ST_OK:
            model, prev = nxt, nxt.Hash
        else:
            prev = f["hash"]  # the chain goes on behind a header that failed: the sticky error shows
    return signers, start, epoch, facts


def test_fold_equals_the_model_on_200_random_vote_chains():
    rng = random.Random(20180417)
    shrunk = failures = 0
    for k in range(200):
        signers, start, epoch, facts = _random_chain(rng)
        want_st, want, want_applied = M.fold(start.copy(), epoch, facts)
        s = lib_snapshot(signers, 0, start.Hash)
        st, applied = lib_fold(s, 1, epoch, facts)
        assert list(st) == want_st, k
        assert applied == want_applied, k
        assert lib_state(s) == want.state(), k
        shrunk += len(want.Signers) < len(signers)
        failures += want_applied < len(facts)
    assert shrunk >= 10 and failures >= 20  # drops that shrink the window, and sticky errors, are really in there


def test_snapshot_calls():
    from gsv import clique as Q
    a, b, c = sorted(_addr(n) for n in "ABC")
    s = Q.Snapshot([c, a, b], 7, B.keccak256(b"h"))
    assert s.signers() == [a, b, c] and s.Number == 7 and s.Hash == B.keccak256(b"h")
    assert s.Recents == {} and s.Votes == [] and s.Tally == {}
    assert s.inturn(7, b) and not s.inturn(7, a) and s.inturn(9, a)  # 7 % 3 == 1
    assert Q.CalcDifficulty(s, c) == 2 and Q.CalcDifficulty(s, a) == 1  # block 8: 8 % 3 == 2
    t = s.copy()
    t.close()
    assert s.signers() == [a, b, c]
    assert not Q.Snapshot([], 0, bytes(32)).inturn(1, a)


def test_snapshot_from_genesis(fx):
    from gsv import clique as Q
    g = bytes.fromhex(fx["chain"]["genesis"])
    s = Q.Snapshot.from_genesis(g)
    assert s.Number == 0 and s.Hash == B.header_hash(g)
    assert s.signers() == sorted(_addr(n) for n in fx["chain"]["signers"])
    with pytest.raises(Q.ErrBadHeaderRLP):
        Q.Snapshot.from_genesis(g[:-1])
    with pytest.raises(Q.ErrMissingVanity):
        Q.Snapshot.from_genesis(B.encode_header(M.real_header(Extra=bytes(31))))
    with pytest.raises(Q.ErrMissingSignature):
        Q.Snapshot.from_genesis(B.encode_header(M.real_header(Extra=bytes(96))))


# ---------------------------------------------------------------- the ABI
def test_new_abi_values_are_declared_and_bound():
    from gsv import _lib, params as P
    txt = open(os.path.join(ROOT, "include", "gsv.h")).read()

    def val(name):
        return int(re.search(r"#define %s (-?\d+)" % name, txt).group(1))

    names = ["CHECKPOINT_BENEFICIARY", "INVALID_VOTE", "CHECKPOINT_VOTE", "MISSING_VANITY", "MISSING_SIGNATURE",
             "EXTRA_SIGNERS", "CHECKPOINT_SIGNERS", "MIX_DIGEST", "UNCLE_HASH", "DIFFICULTY", "INVALID_TIMESTAMP",
             "UNAUTHORIZED", "VOTING_CHAIN"]
    for k, name in enumerate(names):
        assert val("GSV_ST_CLIQUE_" + name) == getattr(_lib, "ST_CLIQUE_" + name) == 41 + k
        assert getattr(_lib, "ST_CLIQUE_" + name) in _lib.STATUS_STRINGS
    assert (M.ST_CHECKPOINT_BENEFICIARY, M.ST_VOTING_CHAIN) == (41, 53)
    assert val("GSV_K_RIDGE") == _lib.K_RIDGE == 39 and val("GSV_ABI_VERSION") == 2
    assert ctypes.sizeof(_lib.CliqueConfigStruct) == 16 and _lib.CLIQUE_RECORD_BYTES == M.REC_BYTES == 128
    assert (P.RinkebyChainConfig.Clique.Period, P.RinkebyChainConfig.Clique.Epoch) == (15, 30000)
    assert (P.AllCliqueProtocolChanges.Clique.Period, P.AllCliqueProtocolChanges.Clique.Epoch) == (0, 30000)
    assert P.MainnetChainConfig.Clique is None


def test_entry_points_check_their_arguments():
    from gsv import _lib
    L = _lib.load()
    E = _lib.E_INVALID_ARG
    assert L.gsv_clique_snapshot_new(None, 1, 0, None) is None
    assert L.gsv_clique_snapshot_signers(None, None, 0) == 0
    h = L.gsv_clique_snapshot_new(None, 0, 0, ctypes.c_char_p(bytes(32)))
    zero_epoch = _lib.CliqueConfigStruct(1, 0)
    st = (ctypes.c_uint8 * 1)()
    assert L.gsv_clique_fold(h, ctypes.byref(zero_epoch), None, 0, None, None, None, None) == E
    ok = _lib.CliqueConfigStruct(1, 8)
    assert L.gsv_clique_fold(h, ctypes.byref(ok), None, 0, None, None, None, None) == 0
    assert L.gsv_clique_fold(h, ctypes.byref(ok), None, 1, None, None, st, None) == E
    L.gsv_clique_snapshot_free(h)
    L.gsv_clique_snapshot_free(None)


# ---------------------------------------------------------------- host code under sanitizers
def test_host_code_as_a_program_under_sanitizers(tmp_path):
    """tests/native/clique_host_main.cpp (layouts, records, the snapshot, the fold, the genesis reader) with ASan +
    UBSan (a plain build where the compiler links neither), run as a child process"""
    src = os.path.join(ROOT, "tests", "native", "clique_host_main.cpp")
    exe = tmp_path / "clique_host_main"
    base = ["g++", "-O2", "-g", "-std=c++17", "-Wall", "-o", str(exe), src]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
