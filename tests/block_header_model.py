"""TEST INFRASTRUCTURE: a Python-integer model of Ethash.VerifyHeaders over RLP-encoded headers, written from the
reference's Go text (file:line in the comments) and independent of the kernels under test (csrc/block_header.hip):
no import of `gsv`, Python big integers throughout.  The RLP stream is tests/tx_rules_model.py's (pinned to the
reference's rule corpus by tests/test_gpu_tx_rules.py); Keccak-256 is the oracle's.

  decode_header      rlp.DecodeBytes into types.Header    core/types/block.go:70-86, rlp/decode.go
  encode_header      rlp.EncodeToBytes(header)            rlp/encode.go
  header_hash / hash_no_nonce                             core/types/block.go:99-122
  calc_difficulty    CalcDifficulty                       consensus/ethash/consensus.go:297-459
  verify_header      verifyHeader without the seal, uncle = false     consensus.go:223-285,
                     consensus/misc/dao.go:47-69, consensus/misc/forks.go:30-43
  verify_headers     verifyHeaderWorker over a segment    consensus.go:152-166 (no known-block short cut)

Status numbers are include/gsv.h's.  Two rules are the library's, not the reference's (gsv.h says so): the width
bounds (ST_HEADER_TOO_WIDE) and ST_UNKNOWN_ANCESTOR for a header behind one that did not decode.
"""
from __future__ import annotations

import tx_rules_model as T
from oracle import oracle as O

(ST_OK, ST_BAD_RLP, ST_INVALID_DIFFICULTY, ST_INVALID_MIX_DIGEST, ST_INVALID_POW) = (0, 8, 16, 17, 18)
(ST_HEADER_TOO_WIDE, ST_UNKNOWN_ANCESTOR, ST_EXTRA_TOO_LONG, ST_FUTURE_BLOCK, ST_ZERO_BLOCK_TIME, ST_WRONG_DIFFICULTY,
 ST_GAS_LIMIT_CAP, ST_GAS_USED, ST_GAS_LIMIT_BOUNDS, ST_INVALID_NUMBER, ST_BAD_PRO_DAO_EXTRA, ST_BAD_NO_DAO_EXTRA,
 ST_FORK_HASH) = range(20, 33)

EMPTY_UNCLE_HASH = bytes.fromhex("1dcc4de8dec75d7aab85b567b6ccd41ad312451b948a7413f0a142fd40d49347")  # block.go:36
DAO_EXTRA = bytes.fromhex("64616f2d686172642d666f726b")  # params/dao.go:28
U64 = (1 << 64) - 1
U256 = (1 << 256) - 1

FIELDS = ("ParentHash", "UncleHash", "Coinbase", "Root", "TxHash", "ReceiptHash", "Bloom", "Difficulty", "Number",
          "GasLimit", "GasUsed", "Time", "Extra", "MixDigest", "Nonce")
_FIXED = {"ParentHash": 32, "UncleHash": 32, "Coinbase": 20, "Root": 32, "TxHash": 32, "ReceiptHash": 32, "Bloom": 256,
          "MixDigest": 32, "Nonce": 8}
_BIG = ("Difficulty", "Number", "Time")
_UINT = ("GasLimit", "GasUsed")


def keccak256(b: bytes) -> bytes:
    return O.keccak256(bytes(b))


def new_header(**kw):
    """a header with the zero values of types.Header, then the given fields"""
    h = {"ParentHash": bytes(32), "UncleHash": EMPTY_UNCLE_HASH, "Coinbase": bytes(20), "Root": bytes(32),
         "TxHash": bytes(32), "ReceiptHash": bytes(32), "Bloom": bytes(256), "Difficulty": 0, "Number": 0, "GasLimit": 0,
         "GasUsed": 0, "Time": 0, "Extra": b"", "MixDigest": bytes(32), "Nonce": bytes(8)}
    h.update(kw)
    return h


def _enc_field(name, v):
    if name in _BIG or name in _UINT:
        return T.enc_uint(int(v))
    return T.enc_string(bytes(v))


def encode_fields(h, names=FIELDS) -> bytes:
    return T.enc_list(b"".join(_enc_field(n, h[n]) for n in names))


def encode_header(h) -> bytes:
    return encode_fields(h)


def decode_header(blob: bytes):
    """rlp.DecodeBytes(blob, &header) -> dict, or raises T.RLPError (makeStructDecoder, rlp/decode.go:432-452)"""
    s = T.Stream(blob, len(blob) if len(blob) else "len")
    s.List()
    h = {}
    for name in FIELDS:
        try:
            if name in _FIXED:
                h[name] = T.decode_byte_array(s, _FIXED[name])
            elif name in _BIG:
                h[name] = T.decode_bigint(s)
            elif name in _UINT:
                h[name] = T.decode_uint(s)
            else:
                h[name] = T.decode_bytes(s)
        except T.RLPError as e:
            if e.name == "EOL":
                raise T.RLPError("too few elements")
            raise
    s.ListEnd()
    if s.rpos < len(s.data):
        raise T.RLPError("ErrMoreThanOneValue")
    return h


def decode_status(blob: bytes):
    """(status, header or None): ST_OK, ST_BAD_RLP, or ST_HEADER_TOO_WIDE for a header that decodes with a
    Difficulty or Time above 32 bytes or a Number above 8"""
    try:
        h = decode_header(blob)
    except T.RLPError:
        return ST_BAD_RLP, None
    if h["Difficulty"] > U256 or h["Time"] > U256 or h["Number"] > U64:
        return ST_HEADER_TOO_WIDE, h
    return ST_OK, h


def header_hash(blob: bytes) -> bytes:  # Header.Hash(): rlpHash(h), block.go:101-103
    return keccak256(blob)


def hash_no_nonce(h) -> bytes:  # block.go:106-122
    return keccak256(encode_fields(h, FIELDS[:13]))


def nonce_number(h) -> int:  # BlockNonce.Uint64(), block.go:56-58
    return int.from_bytes(h["Nonce"], "big")


# ---------------------------------------------------------------- CalcDifficulty
class Config:
    """params.ChainConfig's fields the rules read; None is a nil *big.Int"""

    def __init__(self, homestead=None, dao=None, dao_support=False, eip150=None, eip150_hash=bytes(32), byzantium=None):
        self.homestead, self.dao, self.dao_support = homestead, dao, dao_support
        self.eip150, self.eip150_hash, self.byzantium = eip150, bytes(eip150_hash), byzantium


def _forked(s, head):  # isForked, params/config.go:234-239
    return s is not None and s <= head


def _bomb(x, period):
    if period > 1:  # consensus.go:371-375, :420-424, :451-457
        # 2^(period - 2).  Past 2^256 only "2^256 or more" matters to a caller (no header holds such a difficulty),
        # so an exponent of up to 2^64 / 100000 is not materialised: the value returned is then 2^300 and more
        x += 1 << min(period - 2, 300)
    return x


def calc_difficulty(cfg: Config, time: int, parent) -> int:
    """consensus.go:297-459; Python's // floors as big.Int.Div does for a positive divisor.  Exact below 2^300;
    see _bomb for what is returned above"""
    nxt = parent["Number"] + 1
    pd, pt = parent["Difficulty"], parent["Time"]
    if _forked(cfg.byzantium, nxt):  # :323-377
        x = (time - pt) // 9
        x = (1 if parent["UncleHash"] == EMPTY_UNCLE_HASH else 2) - x
        x = max(x, -99)
        x = max(pd + pd // 2048 * x, 131072)
        fake = parent["Number"] - 2999999 if parent["Number"] >= 2999999 else 0
        return _bomb(x, fake // 100000)
    if _forked(cfg.homestead, nxt):  # :382-426
        x = max(1 - (time - pt) // 10, -99)
        x = max(pd + pd // 2048 * x, 131072)
        return _bomb(x, nxt // 100000)
    adjust = pd // 2048  # :431-459
    x = pd + adjust if time - pt < 13 else pd - adjust
    x = max(x, 131072)
    return max(_bomb(x, nxt // 100000), 131072)


def _int64(v):
    v &= U64
    return v - (1 << 64) if v >> 63 else v


def verify_header(cfg: Config, h, blob_hash: bytes, parent, now: int):
    """(pre-seal status, post-seal status, expected difficulty or None): verifyHeader around the seal check"""
    want = None
    if len(h["Extra"]) > 32:  # :225-227
        return ST_EXTRA_TOO_LONG, ST_OK, want
    if h["Time"] > now + 15:  # :234-236
        return ST_FUTURE_BLOCK, ST_OK, want
    if h["Time"] <= parent["Time"]:  # :238-240
        return ST_ZERO_BLOCK_TIME, ST_OK, want
    want = calc_difficulty(cfg, h["Time"] & U64, parent)  # :242, header.Time.Uint64()
    if want != h["Difficulty"]:
        return ST_WRONG_DIFFICULTY, ST_OK, want
    if h["GasLimit"] > 0x7FFFFFFFFFFFFFFF:  # :248-251
        return ST_GAS_LIMIT_CAP, ST_OK, want
    if h["GasUsed"] > h["GasLimit"]:  # :253-255
        return ST_GAS_USED, ST_OK, want
    diff = _int64(_int64(parent["GasLimit"]) - _int64(h["GasLimit"]))  # :258-266
    if diff < 0:
        diff = _int64(-diff)
    if (diff & U64) >= parent["GasLimit"] // 1024 or h["GasLimit"] < 5000:
        return ST_GAS_LIMIT_BOUNDS, ST_OK, want
    if h["Number"] - parent["Number"] != 1:  # :268-270
        return ST_INVALID_NUMBER, ST_OK, want
    post = ST_OK
    if cfg.dao is not None and cfg.dao <= h["Number"] < cfg.dao + 10:  # misc/dao.go:47-69
        if cfg.dao_support and h["Extra"] != DAO_EXTRA:
            post = ST_BAD_PRO_DAO_EXTRA
        elif not cfg.dao_support and h["Extra"] == DAO_EXTRA:
            post = ST_BAD_NO_DAO_EXTRA
    if post == ST_OK and cfg.eip150 is not None and cfg.eip150 == h["Number"]:  # misc/forks.go:30-43
        if cfg.eip150_hash != bytes(32) and cfg.eip150_hash != blob_hash:
            post = ST_FORK_HASH
    return ST_OK, post, want


def verify_headers(cfg: Config, blobs, parent_blob=None, now=0, seal_status=None, seals=None, detail=False):
    """The status of every header of a segment.  seal_status: per header the status VerifySeal would give (None:
    every seal passes); seals: which headers have their seal checked (None: all).  Returns (status list, expected
    difficulties: int, None where the check was not reached); with detail also the statuses in front of the seal
    check (decode, link, checks 1-8) and behind it (DAO extra-data, fork hash)."""
    dec = [decode_status(b) for b in blobs]
    out, wants, pres, posts = [], [], [], []
    for i, blob in enumerate(blobs):
        st, h = dec[i]
        pre, post, want = st, ST_OK, None
        if st == ST_OK:
            parent = None
            if i == 0:
                if parent_blob:
                    pst, ph = decode_status(parent_blob)
                    # chain.GetHeader(ParentHash, Number - 1), the subtraction in uint64 (consensus.go:155)
                    if pst == ST_OK and header_hash(parent_blob) == h["ParentHash"] and \
                            ph["Number"] == (h["Number"] - 1) & U64:
                        parent = ph
            else:
                pst, ph = dec[i - 1]
                if pst == ST_OK and header_hash(blobs[i - 1]) == h["ParentHash"]:
                    parent = ph
            if parent is None:
                pre = ST_UNKNOWN_ANCESTOR
            else:
                pre, post, want = verify_header(cfg, h, header_hash(blob), parent, now)
        st = pre
        if st == ST_OK and (seals is None or seals[i]) and seal_status is not None:
            st = seal_status[i]
        if st == ST_OK:
            st = post
        out.append(st)
        wants.append(want)
        pres.append(pre)
        posts.append(post)
    return (out, wants, pres, posts) if detail else (out, wants)


def want_row(want) -> bytes:
    """the expected-difficulty row of include/gsv.h: zeros where the check was not reached, 0xFF bytes for 2^256 and
    more"""
    if want is None:
        return bytes(32)
    return b"\xff" * 32 if want > U256 else want.to_bytes(32, "big")
