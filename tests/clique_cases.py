"""TEST INFRASTRUCTURE: the cases of Clique's static rule table (verifyHeader and the parent half of
verifyCascadingFields, clique.go:268-349), one header per rule and adjacent rules violated together to pin the order.
Expectations are written by hand; tests/test_clique_model.py checks them against the model.

A case is a header at block NUMBER (5: no checkpoint; 8: a checkpoint, epoch 8) on top of a valid parent, with some
fields overridden.  `now` is relative to the header's Time; `abs_now` is the clock itself (a uint64); `cut` takes
that many bytes off the end of the encoded header.
"""
import block_header_model as B
import clique_model as M

EPOCH, PERIOD = 8, 5
T0 = 1500000000
SIGNER = M.address(M.key_of("A"))
WRONG_HASH = bytes(range(32))

OK = M.ST_OK


def case(name, expect, number=5, now=0, abs_now=None, parent=None, chain=None, cut=0, **fields):
    return dict(name=name, expect=expect, number=number, now=now, abs_now=abs_now, parent=parent or {}, chain=chain,
                cut=cut, fields=fields)


def ext(n):
    return bytes(n)


CP = dict(number=8)  # a checkpoint
CASES = [
    case("valid", OK),
    # rule 0: the decode
    case("a byte short", M.ST_BAD_RLP, cut=1),
    case("number of 9 bytes", M.ST_HEADER_TOO_WIDE, Number=1 << 64),
    case("difficulty of 33 bytes", M.ST_HEADER_TOO_WIDE, Difficulty=1 << 256),
    case("valid checkpoint", OK, **CP),
    case("now is Time", OK, now=0),
    case("now is Time - 1", M.ST_FUTURE_BLOCK, now=-1),
    case("checkpoint beneficiary", M.ST_CHECKPOINT_BENEFICIARY, Coinbase=b"\x01" * 20, **CP),
    case("beneficiary off a checkpoint is a vote", OK, Coinbase=b"\x01" * 20),
    case("vote nonce", M.ST_INVALID_VOTE, Nonce=bytes(7) + b"\x01"),
    case("vote nonce ff..fe", M.ST_INVALID_VOTE, Nonce=b"\xff" * 7 + b"\xfe"),
    case("authorize vote", OK, Nonce=b"\xff" * 8),
    case("checkpoint vote", M.ST_CHECKPOINT_VOTE, Nonce=b"\xff" * 8, **CP),
    case("vanity 31", M.ST_MISSING_VANITY, Extra=ext(31)),
    case("vanity 0", M.ST_MISSING_VANITY, Extra=b""),
    case("signature 32", M.ST_MISSING_SIGNATURE, Extra=ext(32)),
    case("signature 96", M.ST_MISSING_SIGNATURE, Extra=ext(96)),
    case("extra signers", M.ST_EXTRA_SIGNERS, Extra=ext(117)),
    case("extra signers 98", M.ST_EXTRA_SIGNERS, Extra=ext(98)),
    case("checkpoint signers 19", M.ST_CHECKPOINT_SIGNERS, Extra=ext(97 + 19), **CP),
    case("checkpoint without signers", OK, Extra=ext(97), **CP),  # static only: the list is the fold's to compare
    case("mix digest", M.ST_MIX_DIGEST, MixDigest=bytes(31) + b"\x01"),
    case("uncle hash", M.ST_UNCLE_HASH, UncleHash=bytes(32)),
    case("difficulty 3", M.ST_DIFFICULTY, Difficulty=3),
    case("difficulty 0", M.ST_DIFFICULTY, Difficulty=0),
    case("difficulty 1", OK, Difficulty=1),
    case("difficulty 258", M.ST_DIFFICULTY, Difficulty=258),
    case("fork hash", M.ST_FORK_HASH, chain=dict(eip150=5, eip150_hash=WRONG_HASH)),
    case("fork hash not set", OK, chain=dict(eip150=5)),
    case("fork at another block", OK, chain=dict(eip150=6, eip150_hash=WRONG_HASH)),
    case("broken link", M.ST_UNKNOWN_ANCESTOR, ParentHash=WRONG_HASH),
    case("parent number", M.ST_UNKNOWN_ANCESTOR, Number=6),
    case("time too close", M.ST_INVALID_TIMESTAMP, Time=T0 + PERIOD - 1),
    case("time exactly a period", OK, Time=T0 + PERIOD),
    case("time equals parent", M.ST_INVALID_TIMESTAMP, Time=T0),
    # parent.Time.Uint64() + Period > Time.Uint64(): the parent's low 64 bits are 5
    case("parent time 2^64 + 5, time 10", OK, parent=dict(Time=(1 << 64) + 5), Time=10),
    case("parent time 2^64 + 5, time 9", M.ST_INVALID_TIMESTAMP, parent=dict(Time=(1 << 64) + 5), Time=9),
    # parent.Time + Period wraps to 4
    case("parent time 2^64 - 1 wraps", OK, parent=dict(Time=(1 << 64) - 1), Time=4),
    case("time 2^64 is the future", M.ST_FUTURE_BLOCK, abs_now=(1 << 64) - 1, Time=1 << 64),  # Time in full width
    case("time 2^64 - 1 is now", OK, abs_now=(1 << 64) - 1, Time=(1 << 64) - 1),
    # adjacent rules violated together: the earlier one wins
    case("decode + future", M.ST_HEADER_TOO_WIDE, abs_now=(1 << 64) - 1, Time=1 << 256),
    case("a byte short + future", M.ST_BAD_RLP, now=-1, cut=1),
    case("future + beneficiary", M.ST_FUTURE_BLOCK, now=-1, Coinbase=b"\x01" * 20, **CP),
    case("beneficiary + vote nonce", M.ST_CHECKPOINT_BENEFICIARY, Coinbase=b"\x01" * 20, Nonce=bytes(7) + b"\x01", **CP),
    case("vote nonce + checkpoint vote", M.ST_INVALID_VOTE, Nonce=bytes(7) + b"\x01", **CP),
    case("checkpoint vote + vanity", M.ST_CHECKPOINT_VOTE, Nonce=b"\xff" * 8, Extra=ext(31), **CP),
    case("vanity + mix digest", M.ST_MISSING_VANITY, Extra=ext(31), MixDigest=b"\x01" * 32),
    case("signature + mix digest", M.ST_MISSING_SIGNATURE, Extra=ext(96), MixDigest=b"\x01" * 32),
    case("extra signers + mix digest", M.ST_EXTRA_SIGNERS, Extra=ext(117), MixDigest=b"\x01" * 32),
    case("checkpoint signers + mix digest", M.ST_CHECKPOINT_SIGNERS, Extra=ext(98), MixDigest=b"\x01" * 32, **CP),
    case("mix digest + uncle hash", M.ST_MIX_DIGEST, MixDigest=b"\x01" * 32, UncleHash=bytes(32)),
    case("uncle hash + difficulty", M.ST_UNCLE_HASH, UncleHash=bytes(32), Difficulty=7),
    case("difficulty + fork hash", M.ST_DIFFICULTY, Difficulty=7, chain=dict(eip150=5, eip150_hash=WRONG_HASH)),
    case("fork hash + broken link", M.ST_FORK_HASH, ParentHash=WRONG_HASH, chain=dict(eip150=5, eip150_hash=WRONG_HASH)),
    case("broken link + time too close", M.ST_UNKNOWN_ANCESTOR, ParentHash=WRONG_HASH, Time=T0),
]


def build(c):
    """(chain config, parent blob, header blob, now) of a case"""
    number = c["number"]
    parent = M.real_header(Number=number - 1, Time=T0, Difficulty=1)
    parent.update(c["parent"])
    parent_blob = B.encode_header(M.sign(parent, M.key_of("B")))
    extra = bytes(32) + (SIGNER if number % EPOCH == 0 else b"") + bytes(65)
    h = M.real_header(ParentHash=B.header_hash(parent_blob), Number=number, Time=T0 + PERIOD + 2, Extra=extra)
    h.update(c["fields"])
    if len(h["Extra"]) >= 65:
        h = M.sign(h, M.key_of("A"))
    blob = B.encode_header(h)
    blob = blob[:len(blob) - c["cut"]]
    now = c["abs_now"] if c["abs_now"] is not None else h["Time"] + c["now"]
    return B.Config(**(c["chain"] or {})), parent_blob, blob, now


def genesis_alone():
    """the genesis header on its own: Number 0, no parent, any difficulty"""
    return B.encode_header(M.genesis_header([SIGNER], time=T0))
