"""TEST INFRASTRUCTURE: a Python model of consensus receipts and the logs bloom, written from the reference's Go
text (file:line in the comments) and independent of the kernels under test (csrc/receipt.hip): no import of `gsv`.
The RLP stream is tests/tx_rules_model.py's (pinned to the reference's rule corpus by tests/test_gpu_tx_rules.py);
Keccak-256 is the oracle's.

  encode_receipt / decode_receipt   receiptRLP, rlpLog      core/types/receipt.go:67-128, core/types/log.go:65-95
  bloom9 / logs_bloom / create_bloom / bloom_lookup         core/types/bloom9.go:94-136
  validate           the receipt half of ValidateState      core/block_validator.go:80-95

A receipt is a dict {"status": bytes, "gas": int, "bloom": bytes(256), "logs": [(address20, [topic32, ...], data)]}.
A bloom is the reference's Bloom: 256 bytes, the big-endian bytes of the big.Int (bloom9.go:44-57).
Status numbers are include/gsv.h's.  One rule is the library's, not the reference's (gsv.h says so): a list that
holds a receipt that does not decode reports that receipt's status, with a zero bloom, a zero root and gas 0.
"""
from __future__ import annotations

import tx_rules_model as T
from oracle import oracle as O

(ST_OK, ST_BAD_RLP) = (0, 8)
(ST_RECEIPT_STATUS, ST_GAS_USED_MISMATCH, ST_INVALID_BLOOM, ST_INVALID_RECEIPT_ROOT) = range(33, 37)

BLOOM_BYTES = 256  # BloomByteLength, bloom9.go:33
EMPTY_ROOT = bytes.fromhex("56e81f171bcc55a6ff8345e692c0f86e5b48e01b996cadc001622fb5e363b421")  # types.EmptyRootHash
STATUS_FAILED, STATUS_SUCCESSFUL = b"", b"\x01"  # receiptStatusFailedRLP / SuccessfulRLP, receipt.go:33-34


def keccak256(b: bytes) -> bytes:
    return O.keccak256(bytes(b))


# ---------------------------------------------------------------- RLP
def encode_log(log) -> bytes:  # Log.EncodeRLP, log.go:83-85
    addr, topics, data = log
    return T.enc_list(T.enc_string(addr) + T.enc_list(b"".join(T.enc_string(t) for t in topics)) + T.enc_string(data))


def encode_receipt(r) -> bytes:  # Receipt.EncodeRLP, receipt.go:98-100
    return T.enc_list(T.enc_string(r["status"]) + T.enc_uint(r["gas"]) + T.enc_string(r["bloom"]) +
                      T.enc_list(b"".join(encode_log(g) for g in r["logs"])))


def new_receipt(status=STATUS_SUCCESSFUL, gas=0, logs=(), bloom=None):
    logs = [(bytes(a), [bytes(t) for t in ts], bytes(d)) for a, ts, d in logs]
    return {"status": bytes(status), "gas": int(gas), "logs": logs,
            "bloom": bytes(bloom) if bloom is not None else logs_bloom(logs)}


def _struct(s: T.Stream, fields):
    """makeStructDecoder (rlp/decode.go:432-452): List, each field (EOL -> too few elements), ListEnd (too many)"""
    s.List()
    out = []
    for dec in fields:
        try:
            out.append(dec(s))
        except T.RLPError as e:
            if e.name == "EOL":
                raise T.RLPError("too few elements")
            raise
    s.ListEnd()
    return out


def _slice(s: T.Stream, elem):
    """decodeListSlice / decodeSliceElems (rlp/decode.go:323-368): a list of any number of elements"""
    s.List()
    out = []
    while True:
        try:
            out.append(elem(s))
        except T.RLPError as e:
            if e.name == "EOL":
                break
            raise
    s.ListEnd()
    return out


def _decode_log(s: T.Stream):
    # *Log implements Decoder (log.go:88-95): decodeDecoder calls it for any input, an empty string or list
    # included (rlp/decode.go:541-561), so there is no nil short cut; rlpLog is a struct of three fields
    addr, topics, data = _struct(s, (lambda x: T.decode_byte_array(x, 20),
                                     lambda x: _slice(x, lambda y: T.decode_byte_array(y, 32)), T.decode_bytes))
    return addr, topics, data


def decode_receipt(blob: bytes):
    """rlp.DecodeBytes(blob, &receipt) -> dict, or raises T.RLPError / ValueError("invalid receipt status").
    Receipt.DecodeRLP (receipt.go:104-114): the struct first, then setStatus (:116-128); DecodeBytes refuses
    trailing input last (rlp/decode.go:142-144)."""
    s = T.Stream(blob, len(blob) if len(blob) else "len")
    status, gas, bloom, logs = _struct(s, (T.decode_bytes, T.decode_uint, lambda x: T.decode_byte_array(x, BLOOM_BYTES),
                                           lambda x: _slice(x, _decode_log)))
    if status not in (STATUS_SUCCESSFUL, STATUS_FAILED) and len(status) != 32:
        raise ValueError("invalid receipt status")
    if s.rpos < len(s.data):
        raise T.RLPError("ErrMoreThanOneValue")
    return {"status": status, "gas": gas, "bloom": bloom, "logs": logs}


def decode_status(blob: bytes):
    """(status, receipt or None)"""
    try:
        return ST_OK, decode_receipt(blob)
    except T.RLPError:
        return ST_BAD_RLP, None
    except ValueError:
        return ST_RECEIPT_STATUS, None


# ---------------------------------------------------------------- bloom
def bloom_indexes(b: bytes):
    """the three bit numbers of bloom9(b) (bloom9.go:115-127)"""
    h = keccak256(b)
    return [((h[i] << 8) + h[i + 1]) & 2047 for i in (0, 2, 4)]


def bloom9(b: bytes) -> int:
    r = 0
    for i in bloom_indexes(b):
        r |= 1 << i
    return r


def to_bloom(x: int) -> bytes:  # BytesToBloom(bin.Bytes()), bloom9.go:44-57
    return x.to_bytes(BLOOM_BYTES, "big")


def logs_bloom_int(logs) -> int:  # LogsBloom, bloom9.go:103-113
    r = 0
    for addr, topics, _ in logs:
        r |= bloom9(addr)
        for t in topics:
            r |= bloom9(t)
    return r


def logs_bloom(logs) -> bytes:
    return to_bloom(logs_bloom_int(logs))


def create_bloom(receipts) -> bytes:  # CreateBloom, bloom9.go:94-101: over the receipts' LOGS, not their Bloom fields
    r = 0
    for rc in receipts:
        r |= logs_bloom_int(rc["logs"])
    return to_bloom(r)


def bloom_lookup(bloom: bytes, topic: bytes) -> bool:  # BloomLookup, bloom9.go:131-136
    cmp = bloom9(topic)
    return int.from_bytes(bloom, "big") & cmp == cmp


# ---------------------------------------------------------------- the receipt half of ValidateState
def derive_sha(blobs) -> bytes:  # types.DeriveSha(receipts), derive_sha.go:32-41
    return O.derive_sha([bytes(b) for b in blobs]) if blobs else EMPTY_ROOT


def validate(blobs, want_bloom=None, want_root=None, want_gas=None):
    """(status, bloom, root, gas used, per-receipt statuses) of one list of receipt RLPs; None skips a compare"""
    sts, recs = zip(*(decode_status(b) for b in blobs)) if blobs else ((), ())
    bad = [s for s in sts if s != ST_OK]
    if bad:
        return bad[0], bytes(BLOOM_BYTES), bytes(32), 0, list(sts)
    bloom, root = create_bloom(recs), derive_sha(blobs)
    gas = recs[-1]["gas"] if recs else 0
    st = ST_OK
    if want_gas is not None and want_gas != gas:  # block_validator.go:82-84
        st = ST_GAS_USED_MISMATCH
    elif want_bloom is not None and bytes(want_bloom) != bloom:  # :87-90
        st = ST_INVALID_BLOOM
    elif want_root is not None and bytes(want_root) != root:  # :92-95
        st = ST_INVALID_RECEIPT_ROOT
    return st, bloom, root, gas, list(sts)
