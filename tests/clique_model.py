"""TEST INFRASTRUCTURE: a Python-integer model of consensus/clique over RLP-encoded headers, written from the
reference's Go text (file:line in the comments): the yardstick for a batched Clique.VerifyHeaders, which the library
has only in part (the host fold).  No import of `gsv`; dicts, sets and lists as the reference holds them.  The header codec is
tests/block_header_model.py's; sigHash is keccak(rlp_list(...)) built from the DECODED fields with that encoder, never
by splicing bytes; signatures come from the oracle's libsecp256k1 port with tests/rfc6979_model.py's nonce (what
crypto.Sign computes).

  sig_hash            sigHash                           consensus/clique/clique.go:146-168
  ecrecover           ecrecover (no signature cache)    clique.go:171-193
  verify_static       verifyHeader + the parent half of verifyCascadingFields    clique.go:268-349
  Snapshot            newSnapshot, cast, uncast, apply, signers, inturn          consensus/clique/snapshot.go
  verify_seal         verifySeal behind the snapshot    clique.go:478-502
  verify_headers      Clique.VerifyHeaders over a segment and a snapshot at its parent   clique.go:246-262, :351-367

Status numbers are include/gsv.h's.  Two rules are a batch's, not the reference's (gsv.h says so): a header that did not decode, or
whose ParentHash is not the snapshot's Hash, fails the snapshot walk with ST_UNKNOWN_ANCESTOR (the reference would go
to its database, which a batch call does not have); and a failing apply leaves the snapshot at the last header
applied.
"""
from __future__ import annotations

import copy

import block_header_model as B
import rfc6979_model as R
from oracle import oracle as O

ST_OK, ST_INVALID_RECID, ST_RECOVER_FAILED, ST_BAD_RLP = 0, 3, 4, 8
ST_HEADER_TOO_WIDE, ST_UNKNOWN_ANCESTOR, ST_FUTURE_BLOCK, ST_FORK_HASH = 20, 21, 23, 32
(ST_CHECKPOINT_BENEFICIARY, ST_INVALID_VOTE, ST_CHECKPOINT_VOTE, ST_MISSING_VANITY, ST_MISSING_SIGNATURE,
 ST_EXTRA_SIGNERS, ST_CHECKPOINT_SIGNERS, ST_MIX_DIGEST, ST_UNCLE_HASH, ST_DIFFICULTY, ST_INVALID_TIMESTAMP,
 ST_UNAUTHORIZED, ST_VOTING_CHAIN) = range(41, 54)

EXTRA_VANITY, EXTRA_SEAL = 32, 65  # clique.go:58-59
NONCE_AUTH, NONCE_DROP = b"\xff" * 8, bytes(8)  # clique.go:61-62
EPOCH_LENGTH = 30000  # clique.go:55
U64 = (1 << 64) - 1


class CliqueConfig:
    def __init__(self, period=0, epoch=0):
        self.period, self.epoch = period, epoch or EPOCH_LENGTH  # clique.New, clique.go:216-218


# ---------------------------------------------------------------- keys, sigHash, ecrecover
def key_of(name: str) -> bytes:
    """a fixed secret key per account name (the reference's tester pool draws random ones)"""
    return B.keccak256(b"clique test account " + name.encode())


def address(key: bytes) -> bytes:  # crypto.PubkeyToAddress
    return B.keccak256(O.secp_pubkey(key)[1:])[12:]


def sig_hash(h) -> bytes:  # clique.go:146-168
    g = dict(h)
    g["Extra"] = h["Extra"][:len(h["Extra"]) - EXTRA_SEAL]
    return B.keccak256(B.encode_fields(g))


def sign(h, key: bytes):
    """crypto.Sign(sigHash(header), key) into Extra's last 65 bytes (clique.go:645-650); returns the header"""
    msg = sig_hash(h)
    sig = O.secp_sign(msg, key, R.nonce(key, msg))
    g = dict(h)
    g["Extra"] = h["Extra"][:len(h["Extra"]) - EXTRA_SEAL] + sig
    return g


def ecrecover(h):
    """(status, signer or None): clique.go:171-193"""
    if len(h["Extra"]) < EXTRA_SEAL:
        return ST_MISSING_SIGNATURE, None
    rc, pub = O.ecrecover(sig_hash(h), h["Extra"][-EXTRA_SEAL:])
    if rc == -1:
        return ST_INVALID_RECID, None
    if rc != 1:
        return ST_RECOVER_FAILED, None
    return ST_OK, B.keccak256(pub[1:])[12:]


# ---------------------------------------------------------------- verifyHeader's static half
def verify_static(chain_cfg: B.Config, cfg: CliqueConfig, h, blob_hash: bytes, parent, parent_hash, now: int):
    """verifyHeader (clique.go:268-325) and verifyCascadingFields up to the snapshot (:331-349).  parent: the decoded
    header in front (None: none, or it did not decode), parent_hash its Hash()."""
    number = h["Number"]
    if h["Time"] > now:  # :275
        return ST_FUTURE_BLOCK
    checkpoint = number % cfg.epoch == 0
    if checkpoint and h["Coinbase"] != bytes(20):  # :280
        return ST_CHECKPOINT_BENEFICIARY
    if h["Nonce"] != NONCE_AUTH and h["Nonce"] != NONCE_DROP:  # :284
        return ST_INVALID_VOTE
    if checkpoint and h["Nonce"] != NONCE_DROP:  # :287
        return ST_CHECKPOINT_VOTE
    if len(h["Extra"]) < EXTRA_VANITY:  # :291
        return ST_MISSING_VANITY
    if len(h["Extra"]) < EXTRA_VANITY + EXTRA_SEAL:  # :294
        return ST_MISSING_SIGNATURE
    signers_bytes = len(h["Extra"]) - EXTRA_VANITY - EXTRA_SEAL
    if not checkpoint and signers_bytes != 0:  # :299
        return ST_EXTRA_SIGNERS
    if checkpoint and signers_bytes % 20 != 0:  # :302
        return ST_CHECKPOINT_SIGNERS
    if h["MixDigest"] != bytes(32):  # :306
        return ST_MIX_DIGEST
    if h["UncleHash"] != B.EMPTY_UNCLE_HASH:  # :310
        return ST_UNCLE_HASH
    if number > 0 and h["Difficulty"] not in (1, 2):  # :314
        return ST_DIFFICULTY
    if chain_cfg.eip150 is not None and chain_cfg.eip150 == number:  # misc/forks.go:30-43
        if chain_cfg.eip150_hash != bytes(32) and chain_cfg.eip150_hash != blob_hash:
            return ST_FORK_HASH
    if number == 0:  # :334
        return ST_OK
    if parent is None or parent["Number"] != number - 1 or parent_hash != h["ParentHash"]:  # :344
        return ST_UNKNOWN_ANCESTOR
    if ((parent["Time"] & U64) + cfg.period) & U64 > h["Time"] & U64:  # :347, uint64 arithmetic
        return ST_INVALID_TIMESTAMP
    return ST_OK


# ---------------------------------------------------------------- the facts of one header
def vote_of(nonce: bytes) -> int:
    return 1 if nonce == NONCE_AUTH else 0 if nonce == NONCE_DROP else 2


def facts_of(chain_cfg, cfg, blobs, parent_blob, now):
    """per header what the fold reads, i.e. the record of include/gsv.h ("clique") before it is packed: a dict of
    static status, number, hash, parent hash, signer status, signer, coinbase, vote, difficulty class and Extra.
    `number` follows the record's contract: the header's Number where it fits 8 bytes, 0 for a header that did not
    decode or whose Number is wider (such a header is ST_HEADER_TOO_WIDE, so the 0 never stands for a genesis: fold
    tests `decoded` and the static status before it reads the number)."""
    dec = [B.decode_status(b) for b in blobs]
    out = []
    for i, blob in enumerate(blobs):
        st, h = dec[i]
        f = dict(static=st, decoded=h is not None, number=0, hash=bytes(32), parent_hash=bytes(32), signer_status=
                 ST_MISSING_SIGNATURE, signer=bytes(20), coinbase=bytes(20), vote=0, difficulty=0, extra=b"", extra_off=0,
                 sighash=bytes(32), sig=bytes(65))
        if h is not None:
            sst, signer = ecrecover(h)
            f.update(number=h["Number"] if h["Number"] <= U64 else 0,
                     hash=B.header_hash(blob), parent_hash=h["ParentHash"], signer_status=sst,
                     signer=signer or bytes(20), coinbase=h["Coinbase"], vote=vote_of(h["Nonce"]),
                     difficulty=h["Difficulty"] if h["Difficulty"] in (1, 2) else 0, extra=h["Extra"],
                     extra_off=len(blob) - 42 - len(h["Extra"]))
            if len(h["Extra"]) >= EXTRA_SEAL:
                f.update(sighash=sig_hash(h), sig=h["Extra"][-EXTRA_SEAL:])
        if st == ST_OK:
            if i == 0:
                pst, ph = B.decode_status(parent_blob) if parent_blob else (ST_BAD_RLP, None)
                par, phash = (ph, B.header_hash(parent_blob)) if pst == ST_OK else (None, None)
            else:
                pst, ph = dec[i - 1]
                par, phash = (ph, B.header_hash(blobs[i - 1])) if pst == ST_OK else (None, None)
            f["static"] = verify_static(chain_cfg, cfg, h, f["hash"], par, phash, now)
        out.append(f)
    return out


REC_BYTES = 128


def record_bytes(f) -> bytes:
    """the 128-byte record of include/gsv.h ("clique") for one header's facts"""
    r = (f["hash"] + f["parent_hash"] + f["signer"] + f["coinbase"] + f["number"].to_bytes(8, "little") +
         f["extra_off"].to_bytes(4, "little") + len(f["extra"]).to_bytes(4, "little") +
         bytes([f["static"], f["signer_status"], f["vote"], f["difficulty"]]) + bytes(4))
    assert len(r) == REC_BYTES
    return r


# ---------------------------------------------------------------- the snapshot
class Snapshot:
    """snapshot.go:46-76.  Signers: set; Recents: {block: signer}; Votes: list of dicts in order; Tally:
    {address: [authorize, votes]}"""

    def __init__(self, signers=(), number=0, hash=bytes(32)):
        self.Number, self.Hash = number, bytes(hash)
        self.Signers = set(bytes(s) for s in signers)
        self.Recents, self.Votes, self.Tally = {}, [], {}

    def copy(self):
        return copy.deepcopy(self)

    def signers(self):  # :288-301
        return sorted(self.Signers)

    def inturn(self, number, signer):  # :304-310
        # ZeroDivisionError for an empty signer set, where the reference panics too (integer divide by zero);
        # TestVoting's "single signer, dropping itself" leaves such a snapshot and never asks
        s = self.signers()
        offset = 0
        while offset < len(s) and s[offset] != signer:
            offset += 1
        return number % len(s) == offset

    def valid_vote(self, address, authorize):  # :131-134
        signer = address in self.Signers
        return (signer and not authorize) or (not signer and authorize)

    def cast(self, address, authorize):  # :137-150
        if not self.valid_vote(address, authorize):
            return False
        if address in self.Tally:
            self.Tally[address][1] += 1
        else:
            self.Tally[address] = [authorize, 1]
        return True

    def uncast(self, address, authorize):  # :153-171
        if address not in self.Tally:
            return False
        t = self.Tally[address]
        if t[0] != authorize:
            return False
        if t[1] > 1:
            t[1] -= 1
        else:
            del self.Tally[address]
        return True

    def state(self):
        """what the tests compare against the library's snapshot"""
        return dict(number=self.Number, hash=self.Hash, signers=self.signers(), recents=dict(self.Recents),
                    votes=[(v["Signer"], v["Block"], v["Address"], v["Authorize"]) for v in self.Votes],
                    tally={a: (t[0], t[1]) for a, t in self.Tally.items()})


def apply_one(s: Snapshot, epoch: int, f):
    """one header of Snapshot.apply (snapshot.go:192-280) on a copy: (new snapshot, ST_OK) or (None, error).  The
    walk of snapshot() in front of it: ST_UNKNOWN_ANCESTOR for a header that did not decode or does not link (OURS),
    ST_VOTING_CHAIN for a number that does not follow (:181-188)."""
    if f["static"] in (ST_BAD_RLP, ST_HEADER_TOO_WIDE) or f["parent_hash"] != s.Hash:
        return None, ST_UNKNOWN_ANCESTOR
    number = f["number"]
    if number != s.Number + 1:
        return None, ST_VOTING_CHAIN
    snap = s.copy()
    if number % epoch == 0:  # :195-198
        snap.Votes, snap.Tally = [], {}
    limit = len(snap.Signers) // 2 + 1  # :200-202
    if number >= limit:
        snap.Recents.pop(number - limit, None)
    if f["signer_status"] != ST_OK:  # :204-207
        return None, f["signer_status"]
    signer = f["signer"]
    if signer not in snap.Signers:  # :208-210
        return None, ST_UNAUTHORIZED
    if signer in snap.Recents.values():  # :211-215
        return None, ST_UNAUTHORIZED
    snap.Recents[number] = signer
    for i, vote in enumerate(snap.Votes):  # :219-228
        if vote["Signer"] == signer and vote["Address"] == f["coinbase"]:
            snap.uncast(vote["Address"], vote["Authorize"])
            del snap.Votes[i]
            break
    if f["vote"] == 2:  # :231-238
        return None, ST_INVALID_VOTE
    authorize = f["vote"] == 1
    if snap.cast(f["coinbase"], authorize):  # :239-246
        snap.Votes.append(dict(Signer=signer, Block=number, Address=f["coinbase"], Authorize=authorize))
    t = snap.Tally.get(f["coinbase"])
    if t is not None and t[1] > len(snap.Signers) // 2:  # :248-279
        if t[0]:
            snap.Signers.add(f["coinbase"])
        else:
            snap.Signers.discard(f["coinbase"])
            limit = len(snap.Signers) // 2 + 1
            if number >= limit:
                snap.Recents.pop(number - limit, None)
            i = 0
            while i < len(snap.Votes):
                if snap.Votes[i]["Signer"] == f["coinbase"]:
                    snap.uncast(snap.Votes[i]["Address"], snap.Votes[i]["Authorize"])
                    del snap.Votes[i]
                    i -= 1
                i += 1
        snap.Votes = [v for v in snap.Votes if v["Address"] != f["coinbase"]]
        snap.Tally.pop(f["coinbase"], None)
    snap.Number = number
    snap.Hash = f["hash"]
    return snap, ST_OK


def verify_seal(s: Snapshot, f):  # clique.go:478-502
    if f["signer_status"] != ST_OK:
        return f["signer_status"]
    signer, number = f["signer"], f["number"]
    if signer not in s.Signers:
        return ST_UNAUTHORIZED
    for seen, recent in s.Recents.items():
        if recent == signer:
            limit = len(s.Signers) // 2 + 1
            if seen > (number - limit) & U64:
                return ST_UNAUTHORIZED
    inturn = s.inturn(number, signer)
    if inturn and f["difficulty"] != 2:
        return ST_DIFFICULTY
    if not inturn and f["difficulty"] != 1:
        return ST_DIFFICULTY
    return ST_OK


def fold(s: Snapshot, epoch: int, facts):
    """(status list, snapshot after the last header applied, applied).  Per header: its static status if that is not
    ST_OK; else ST_OK for the genesis header (clique.go:334), which is never applied; else the sticky error of an
    earlier failed apply (:351-354); else the checkpoint's signer list (:356-365) and verifySeal.  Then the header is
    applied whatever its own verdict, as the reference applies a parent that failed verifyHeader."""
    err, applied, out = ST_OK, 0, []
    for f in facts:
        st = f["static"]
        if st == ST_OK and f["number"] != 0:
            if err != ST_OK:
                st = err  # snapshot() failed on an earlier header, clique.go:351-354
            else:
                if f["number"] % epoch == 0:  # :356-365
                    extra = f["extra"]
                    if extra[EXTRA_VANITY:len(extra) - EXTRA_SEAL] != b"".join(s.signers()):
                        st = ST_CHECKPOINT_SIGNERS
                if st == ST_OK:
                    st = verify_seal(s, f)
        out.append(st)
        genesis = f["decoded"] and f["static"] != ST_HEADER_TOO_WIDE and f["number"] == 0
        if err == ST_OK and not genesis:
            nxt, err = apply_one(s, epoch, f)
            if err == ST_OK:
                s = nxt
                applied += 1
    return out, s, applied


def verify_headers(chain_cfg, cfg: CliqueConfig, blobs, snap: Snapshot, parent_blob=None, now=0):
    facts = facts_of(chain_cfg, cfg, blobs, parent_blob, now)
    st, s, applied = fold(snap, cfg.epoch, facts)
    return st, s, applied, facts


# ---------------------------------------------------------------- chains
def voting_headers(scn):
    """the headers TestVoting builds for one scenario (snapshot_test.go:359-374): Number j + 1, Time j * 15, Coinbase
    the voted account's address (the account named "" where no one is voted on), Extra of 97 bytes, every other
    field the zero value (a nil Difficulty encodes as 80), each hash-linked to the one in front"""
    blobs, prev = [], bytes(32)
    for j, v in enumerate(scn["votes"]):
        h = B.new_header(ParentHash=prev, UncleHash=bytes(32), Number=j + 1, Time=j * 15,
                         Coinbase=address(key_of(v.get("voted", ""))), Extra=bytes(EXTRA_VANITY + EXTRA_SEAL),
                         Nonce=NONCE_AUTH if v.get("auth") else NONCE_DROP)
        blob = B.encode_header(sign(h, key_of(v["signer"])))
        blobs.append(blob)
        prev = B.header_hash(blob)
    return blobs


def real_header(**kw):
    """a header with fields of the sizes a Rinkeby header has"""
    h = B.new_header(Root=B.keccak256(b"root"), TxHash=B.keccak256(b"tx"), ReceiptHash=B.keccak256(b"receipt"),
                     Bloom=bytes(range(256)), Difficulty=2, GasLimit=4712388, GasUsed=21000 * 3, Time=1500000000,
                     Extra=bytes(EXTRA_VANITY + EXTRA_SEAL))
    h.update(kw)
    return h


def genesis_header(signers, time=1500000000):
    extra = bytes(EXTRA_VANITY) + b"".join(sorted(signers)) + bytes(EXTRA_SEAL)
    return real_header(Number=0, Difficulty=1, Time=time, Extra=extra)


VANITY = b"gsv".ljust(EXTRA_VANITY, b"\0")


def chain_step(snap: Snapshot, step, prev_time, epoch, period):
    """One valid header on top of `snap` (which stands at its parent) and the snapshot behind it.  step: {signer: name,
    voted: name or absent, auth: bool}.  Difficulty follows the turn, a checkpoint carries the snapshot's signer list
    and casts no vote, Time steps by `period`.  Returns (blob, snapshot)."""
    number = snap.Number + 1
    key = key_of(step["signer"])
    checkpoint = number % epoch == 0
    voted = step.get("voted") if not checkpoint else None
    h = real_header(ParentHash=snap.Hash, Number=number, Time=prev_time + period,
                    Extra=VANITY + (b"".join(snap.signers()) if checkpoint else b"") + bytes(EXTRA_SEAL),
                    Difficulty=2 if snap.inturn(number, address(key)) else 1,
                    Coinbase=address(key_of(voted)) if voted else bytes(20),
                    Nonce=NONCE_AUTH if voted and step.get("auth") else NONCE_DROP)
    blob = B.encode_header(sign(h, key))
    f = facts_of(B.Config(), CliqueConfig(period, epoch), [blob], None, 1 << 62)[0]
    nxt, err = apply_one(snap, epoch, f)
    assert err == ST_OK, (number, err)
    return blob, nxt


def build_chain(plan, signers, epoch, period, genesis_blob):
    """A valid chain on top of a genesis, one chain_step per entry of the plan.  Returns (blobs, the model snapshot
    after each header)."""
    snap = Snapshot(signers, 0, B.header_hash(genesis_blob))
    t = B.decode_header(genesis_blob)["Time"]
    blobs, snaps = [], []
    for step in plan:
        blob, snap = chain_step(snap, step, t, epoch, period)
        t += period
        blobs.append(blob)
        snaps.append(snap)
    return blobs, snaps
