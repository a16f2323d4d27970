"""TEST INFRASTRUCTURE: the receipt cases shared by tests/test_receipt_cpu.py, tests/test_gpu_receipts.py and
tests/golden/make_receipts.py.  Built on tests/receipt_model.py alone (no import of `gsv`); every expected status
here is written by hand from the reference's decoder rules and checked against the model by the CPU test."""
from __future__ import annotations

import random

import receipt_model as R
import tx_rules_model as T

OK, BAD, STATUS = R.ST_OK, R.ST_BAD_RLP, R.ST_RECEIPT_STATUS


def addr(k):
    return bytes([(k * 7 + j) & 255 for j in range(20)])


def topic(k):
    return bytes([(k * 13 + 5 * j + 1) & 255 for j in range(32)])


def log(k, ntopics=1, data=b""):
    return addr(k), [topic(k * 8 + j) for j in range(ntopics)], bytes(data)


def raw(status=None, gas=None, bloom=None, logs=None, extra=b"", tail=b""):
    """a receipt from already-encoded fields; `extra`: further elements of the list, `tail`: bytes behind it"""
    return T.enc_list((T.enc_string(b"\x01") if status is None else status) + (T.enc_uint(21000) if gas is None else gas) +
                      (T.enc_string(bytes(256)) if bloom is None else bloom) + (T.enc_list(b"") if logs is None else logs) +
                      extra) + tail


def raw_log(address=None, topics=None, data=None, extra=b""):
    return T.enc_list((T.enc_string(addr(1)) if address is None else address) +
                      (T.enc_list(T.enc_string(topic(1))) if topics is None else topics) +
                      (T.enc_string(b"data") if data is None else data) + extra)


def with_logs_payload(target: int) -> bytes:
    """a receipt whose Logs list has a payload of exactly `target` bytes: a log without topics whose data is sized
    to fit, behind a smallest log where one log alone cannot have that length (a head grows by a byte at 56)"""
    for first in ([], [(addr(2), [], b"")]):
        for n in range(2, target):
            logs = first + [(addr(3), [], bytes([0x55]) * n)]
            if sum(len(R.encode_log(g)) for g in logs) == target:
                return R.encode_receipt(R.new_receipt(gas=target, logs=logs))
    raise AssertionError(target)


def good_shapes():
    """(name, blob) of receipts that decode: every shape of logs, topics, data, status and gas the issue lists"""
    out = [("no logs", R.new_receipt(gas=1)),
           ("0 topics", R.new_receipt(gas=2, logs=[log(1, 0)])),
           ("4 topics", R.new_receipt(gas=3, logs=[log(2, 4, b"abc")])),
           ("7 topics", R.new_receipt(gas=4, logs=[log(3, 7, b"abc")])),
           ("two logs", R.new_receipt(gas=5, logs=[log(4, 2), log(5, 3, b"\x01" * 40)]))]
    for name, data in (("data 0", b""), ("data 7f", b"\x7f"), ("data 00", b"\x00"), ("data 80", b"\x80"),
                       ("data ff", b"\xff")):
        out.append((name, R.new_receipt(gas=6, logs=[log(6, 1, data)])))
    for n in (55, 56, 255, 256, 65536):
        out.append((f"data {n}", R.new_receipt(gas=n, logs=[log(7, 2, bytes([n & 255]) * n)])))
    for name, st in (("status {}", b""), ("status 01", b"\x01"), ("status 32", bytes(range(32)))):
        out.append((name, R.new_receipt(status=st, gas=7, logs=[log(8)])))
    for g in (0, 0x7F, 0x80, 0xFFFF, (1 << 64) - 1):
        out.append((f"gas {g:#x}", R.new_receipt(gas=g, logs=[log(9)])))
    out.append(("bloom field not the logs'", R.new_receipt(gas=8, logs=[log(10)], bloom=b"\xa5" * 256)))
    blobs = [(name, R.encode_receipt(r)) for name, r in out]
    for target in (54, 55, 56, 57, 254, 255, 256, 257):
        blobs.append((f"logs payload {target}", with_logs_payload(target)))
    return blobs


def decode_corpus():
    """(name, blob, expected status): the good shapes, the status and gas refusals, and one case for each thing
    the reference's decoder refuses"""
    s, u, L = T.enc_string, T.enc_uint, T.enc_list
    cases = [(n, b, OK) for n, b in good_shapes()]
    # setStatus (receipt.go:116-128)
    for name, st in (("status 00", b"\x00"), ("status 02", b"\x02"), ("status 31 bytes", bytes(31)),
                     ("status 33 bytes", bytes(33)), ("status 2 bytes", b"\x01\x01")):
        cases.append((name, raw(status=s(st)), STATUS))
    # the reference judges the status before it looks behind the list, and after the whole struct
    cases.append(("bad status and bytes behind", raw(status=s(b"\x02"), tail=b"\x00"), STATUS))
    cases.append(("bad status and a bad log", raw(status=s(b"\x02"), logs=L(raw_log(address=s(bytes(19))))), BAD))
    # decodeUint
    cases += [("gas 9 bytes", raw(gas=s(bytes([1]) + bytes(8))), BAD),
              ("gas leading zero", raw(gas=s(b"\x00\x01")), BAD),
              ("gas single zero byte", raw(gas=b"\x00"), BAD),
              ("gas 81 05", raw(gas=b"\x81\x05"), BAD),
              ("gas a list", raw(gas=L(b"\x01")), BAD)]
    # non-canonical sizes
    cases += [("data b8 05", raw(logs=L(raw_log(data=b"\xb8\x05hello"))), BAD),
              ("data 81 05", raw(logs=L(raw_log(data=b"\x81\x05"))), BAD),
              ("data b9 00 38", raw(logs=L(raw_log(data=b"\xb9\x00\x38" + bytes(56)))), BAD),
              ("logs f8 for a short list", raw(logs=b"\xf8\x00"), BAD),
              ("receipt f8 with leading zero", b"\xf9\x00" + raw()[1:], BAD),
              ("status 81 01", raw(status=b"\x81\x01"), BAD)]
    # a string where a list belongs, or the reverse
    cases += [("receipt is a string", s(raw()), BAD),
              ("logs is a string", raw(logs=s(b"")), BAD),
              ("a log is a string", raw(logs=L(s(raw_log()[1:]))), BAD),
              ("a log is the empty string", raw(logs=L(b"\x80")), BAD),
              ("topics is a string", raw(logs=L(raw_log(topics=s(b"")))), BAD),
              ("status is a list", raw(status=L(b"")), BAD),
              ("bloom is a list", raw(bloom=L(bytes(256))), BAD),
              ("address is a list", raw(logs=L(raw_log(address=L(bytes(20))))), BAD),
              ("a topic is a list", raw(logs=L(raw_log(topics=L(L(bytes(32)))))), BAD),
              ("data is a list", raw(logs=L(raw_log(data=L(b"")))), BAD)]
    # too few or too many elements
    cases += [("receipt of three", L(s(b"\x01") + u(5) + s(bytes(256))), BAD),
              ("receipt of five", raw(extra=b"\x80"), BAD),
              ("receipt empty list", b"\xc0", BAD),
              ("log of two", raw(logs=L(L(s(addr(1)) + L(b"")))), BAD),
              ("log of four", raw(logs=L(raw_log(extra=b"\x80"))), BAD),
              ("log empty list", raw(logs=L(b"\xc0")), BAD)]
    # fixed widths
    cases += [("bloom 255", raw(bloom=s(bytes(255))), BAD), ("bloom 257", raw(bloom=s(bytes(257))), BAD),
              ("bloom empty", raw(bloom=b"\x80"), BAD),
              ("address 19", raw(logs=L(raw_log(address=s(bytes(19))))), BAD),
              ("address 21", raw(logs=L(raw_log(address=s(bytes(21))))), BAD),
              ("topic 31", raw(logs=L(raw_log(topics=L(s(bytes(31)))))), BAD),
              ("topic 33", raw(logs=L(raw_log(topics=L(s(topic(1)) + s(bytes(33)))))), BAD),
              ("topic empty", raw(logs=L(raw_log(topics=L(b"\x80")))), BAD)]
    # bytes behind the list, an empty item, sizes past their list or the input
    good = R.encode_receipt(R.new_receipt(gas=9, logs=[log(11, 2, b"xyz")]))
    cases += [("bytes behind the list", good + b"\x00", BAD),
              ("a second receipt behind", good + good, BAD),
              ("empty item", b"", BAD),
              ("truncated by one", good[:-1], BAD),
              ("truncated head", good[:2], BAD),
              ("data past its log", raw(logs=L(L(s(addr(1)) + L(b"") + b"\x85ab"))), BAD),
              ("log past the logs list", raw(logs=b"\xc2" + raw_log()), BAD),
              ("single byte", b"\x01", BAD)]
    return cases


def random_receipt(rng: random.Random, max_logs=6):
    logs = []
    for _ in range(rng.randrange(max_logs + 1)):
        nt = rng.choice((0, 1, 1, 2, 3, 4, 4, 7))
        data = bytes(rng.getrandbits(8) for _ in range(rng.choice((0, 1, 5, 32, 55, 56, 64, 100, 300))))
        logs.append((bytes(rng.getrandbits(8) for _ in range(20)),
                     [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(nt)], data))
    status = rng.choice((b"", b"\x01", bytes(rng.getrandbits(8) for _ in range(32))))
    return R.new_receipt(status=status, gas=rng.getrandbits(rng.choice((0, 7, 8, 24, 64))), logs=logs)


def random_lists(seed: int, sizes, max_logs=6):
    """lists of random valid receipts with ascending cumulative gas"""
    rng = random.Random(seed)
    out = []
    for n in sizes:
        lst, gas = [], 0
        for _ in range(n):
            r = random_receipt(rng, max_logs)
            gas += 21000 + rng.randrange(100000)
            r["gas"] = gas
            lst.append(R.encode_receipt(r))
        out.append(lst)
    return out


def count_items(blobs):
    return sum(len(g[1]) + 1 for b in blobs for g in R.decode_receipt(b)["logs"])
