"""TEST INFRASTRUCTURE: the header cases tests/test_block_header_cpu.py and tests/test_gpu_block_header.py share,
built with the model (tests/block_header_model.py) from the fixture's chains (tests/golden/block_headers.json).
Every expectation that is not the model's verdict is written here by hand, so that the CPU tests check the model
against it and the GPU tests check the library against both."""
from __future__ import annotations

import block_header_model as B
import tx_rules_model as T

U64 = (1 << 64) - 1


def config_of(d) -> B.Config:
    return B.Config(homestead=d["homestead"], dao=d["dao"], dao_support=d["dao_support"], eip150=d["eip150"],
                    eip150_hash=bytes.fromhex(d["eip150_hash"]), byzantium=d["byzantium"])


TEST_CONFIG = B.Config(homestead=0, eip150=0, byzantium=0)  # params.TestChainConfig


def base_header():
    """a plain header with every byte of its fixed fields distinct from its neighbours"""
    return B.new_header(ParentHash=bytes(range(1, 33)), UncleHash=bytes(range(33, 65)), Coinbase=bytes(range(65, 85)),
                        Root=bytes(range(85, 117)), TxHash=bytes(range(117, 149)), ReceiptHash=bytes(range(149, 181)),
                        Bloom=bytes((7 * k + 3) & 0xFF for k in range(256)), Difficulty=0x20000, Number=1,
                        GasLimit=0x2FEFD8, GasUsed=0x5208, Time=0x5506EB07, Extra=b"", MixDigest=bytes(range(181, 213)),
                        Nonce=bytes(range(213, 221)))


def with_total(total: int):
    """base_header with Extra sized for an encoding of exactly `total` bytes"""
    h = base_header()
    for _ in range(4):  # the list head and Extra's own head move with the length
        have = len(B.encode_header(h))
        if have == total:
            return h
        h["Extra"] = bytes((5 * k + 0x80) & 0xFF for k in range(len(h["Extra"]) + total - have))
    raise ValueError("no Extra gives %d bytes" % total)


INT_EDGES = (0, 1, 0x7F, 0x80, 1 << 56, U64)


def length_sweep():
    """headers (dicts) over every length the fields allow: Extra 0 .. 33, Difficulty of 1 .. 32 bytes, the integer
    fields at their edges, the 136-byte block edges of both sponges (Hash: 543, 544, 545 bytes; HashNoNonce: 585,
    586, 587, i.e. headers of 627, 628, 629), and the payloads around 2^16 where the two list heads differ"""
    out = []
    for n in range(34):
        out.append(dict(base_header(), Extra=bytes((3 * k + 0x81) & 0xFF for k in range(n))))
    out.append(dict(base_header(), Extra=b"\x05"))  # a single byte below 0x80 encodes as itself
    for n in range(1, 33):
        out.append(dict(base_header(), Difficulty=(0xA5 << (8 * (n - 1))) | (n - 1)))
        out.append(dict(base_header(), Time=(1 << (8 * n)) - 1))
    for v in INT_EDGES:
        for name in ("Difficulty", "Number", "GasLimit", "GasUsed", "Time"):
            out.append(dict(base_header(), **{name: v}))
    for total in (543, 544, 545, 627, 628, 629, 679, 680, 681):
        out.append(with_total(total))
    for payload in (65535, 65536, 65536 + 41, 65536 + 42):
        out.append(with_total(payload + (3 if payload < 65536 else 4)))
    return out


# ---------------------------------------------------------------- the decode corpus
def _fields(h):
    return [B._enc_field(n, h[n]) for n in B.FIELDS]


def _list(items, head=None, tail=b""):
    payload = b"".join(items)
    return (T.enc_head(len(payload), 0xC0, 0xF7) if head is None else head) + payload + tail


def decode_corpus():
    """(name, blob, status) with the status written by hand: ST_OK 0, ST_BAD_RLP 8, ST_HEADER_TOO_WIDE 20"""
    OK, BAD, WIDE = B.ST_OK, B.ST_BAD_RLP, B.ST_HEADER_TOO_WIDE
    h = base_header()
    f = _fields(h)
    ix = {n: k for k, n in enumerate(B.FIELDS)}
    good = _list(f)
    assert good == B.encode_header(h)

    def sub(name, enc):
        g = list(f)
        g[ix[name]] = enc
        return _list(g)

    def raw(b):  # a string head for any content, canonical or not
        return T.enc_head(len(b), 0x80, 0xB7) + b
    cases = [("valid", good, OK),
             ("empty input", b"", BAD),
             ("an empty list", b"\xc0", BAD),
             ("14 items", _list(f[:14]), BAD),
             ("16 items", _list(f + [b"\x80"]), BAD),
             ("a trailing byte", good + b"\x00", BAD),
             ("a trailing byte inside the head's count", _list(f, head=T.enc_head(len(good) - 3 + 1, 0xC0, 0xF7),
                                                              tail=b"\x80"), BAD),
             ("truncated by one byte", good[:-1], BAD),
             ("truncated inside the bloom", good[:300], BAD),
             ("only the list head", good[:3], BAD),
             ("half a list head", good[:2], BAD),
             ("a list head that promises more", _list(f, head=T.enc_head(len(good) - 3 + 1, 0xC0, 0xF7)), BAD),
             ("a list head that promises less", _list(f, head=T.enc_head(len(good) - 3 - 1, 0xC0, 0xF7)), BAD),
             ("a string where the list belongs", b"\xb9" + good[1:], BAD),
             ("a list head with a leading zero", b"\xfa\x00" + good[1:3] + good[3:], BAD),
             ("a 31-byte ParentHash", sub("ParentHash", raw(bytes(31))), BAD),
             ("a 33-byte ParentHash", sub("ParentHash", raw(bytes(33))), BAD),
             ("a 31-byte MixDigest", sub("MixDigest", raw(bytes(31))), BAD),
             ("a 33-byte MixDigest", sub("MixDigest", raw(bytes(33))), BAD),
             ("a 33-byte UncleHash", sub("UncleHash", raw(bytes(33))), BAD),
             ("a 19-byte Coinbase", sub("Coinbase", raw(bytes(19))), BAD),
             ("a 7-byte Nonce", sub("Nonce", raw(bytes(7))), BAD),
             ("a 9-byte Nonce", sub("Nonce", raw(bytes(9))), BAD),
             ("a 255-byte Bloom", sub("Bloom", raw(bytes(255))), BAD),
             ("a 257-byte Bloom", sub("Bloom", raw(bytes(257))), BAD),
             ("a one-byte ParentHash", sub("ParentHash", b"\x05"), BAD),
             ("a hash in the long form", sub("Root", b"\xb8\x20" + bytes(32)), BAD),
             ("a leading zero in Difficulty", sub("Difficulty", raw(b"\x00\x02\x00\x00")), BAD),
             ("a leading zero in Number", sub("Number", raw(b"\x00\x01")), BAD),
             ("a leading zero in GasLimit", sub("GasLimit", raw(b"\x00\x2f\xef\xd8")), BAD),
             ("a leading zero in GasUsed", sub("GasUsed", raw(b"\x00\x52\x08")), BAD),
             ("a leading zero in Time", sub("Time", raw(b"\x00\x55\x06\xeb\x07")), BAD),
             ("Number as the byte 00", sub("Number", b"\x00"), BAD),
             ("GasUsed as the byte 00", sub("GasUsed", b"\x00"), BAD),
             ("81 05 as Number", sub("Number", b"\x81\x05"), BAD),
             ("81 05 as GasUsed", sub("GasUsed", b"\x81\x05"), BAD),
             ("81 05 as Difficulty", sub("Difficulty", b"\x81\x05"), BAD),
             ("81 05 as Extra", sub("Extra", b"\x81\x05"), BAD),
             ("81 80 as Extra", sub("Extra", b"\x81\x80"), OK),
             ("05 as Extra", sub("Extra", b"\x05"), OK),
             ("a 9-byte GasLimit", sub("GasLimit", raw(b"\x01" + bytes(8))), BAD),
             ("a 9-byte GasUsed", sub("GasUsed", raw(b"\x01" + bytes(8))), BAD),
             ("an 8-byte GasLimit", sub("GasLimit", raw(b"\xff" * 8)), OK),
             ("an empty list as Extra", sub("Extra", b"\xc0"), BAD),
             ("an empty list as Number", sub("Number", b"\xc0"), BAD),
             ("a list of 32 bytes as ParentHash", sub("ParentHash", b"\xe0" + bytes(32)), BAD),
             ("a list as Nonce", sub("Nonce", b"\xc8" + bytes(8)), BAD),
             ("Extra in the long form for 55 bytes", sub("Extra", b"\xb8\x37" + bytes(55)), BAD),
             ("Extra of 55 bytes", sub("Extra", raw(bytes(55))), OK),
             ("Extra of 56 bytes", sub("Extra", raw(bytes(56))), OK),
             ("Extra's length with a leading zero", sub("Extra", b"\xb9\x00\x38" + bytes(56)), BAD),
             ("Extra reaching past the list", _list(f[:12] + [b"\xb8\xff" + bytes(40)]), BAD),
             ("Extra swallowing MixDigest and Nonce", _list(f[:12] + [raw(bytes(60))]), BAD),
             ("a length of eight bytes", sub("Extra", b"\xbf" + b"\x01" + bytes(7)), BAD),
             ("a 32-byte Difficulty", sub("Difficulty", raw(b"\xff" * 32)), OK),
             ("a 33-byte Difficulty", sub("Difficulty", raw(b"\x01" + bytes(32))), WIDE),
             ("a 32-byte Time", sub("Time", raw(b"\x80" + bytes(31))), OK),
             ("a 33-byte Time", sub("Time", raw(b"\x01" + bytes(32))), WIDE),
             ("an 8-byte Number", sub("Number", raw(b"\xff" * 8)), OK),
             ("a 9-byte Number", sub("Number", raw(b"\x01" + bytes(8))), WIDE),
             ("a 60-byte Difficulty", sub("Difficulty", raw(b"\x01" + bytes(59))), WIDE)]
    # a wide field in front of a malformed one: the reference's decoder refuses the header
    g = list(f)
    g[ix["Difficulty"]] = raw(b"\x01" + bytes(32))
    g[ix["Nonce"]] = raw(bytes(7))
    cases.append(("a 33-byte Difficulty and a 7-byte Nonce", _list(g), BAD))
    g = list(f)
    g[ix["Number"]] = raw(b"\x01" + bytes(8))
    g[ix["GasLimit"]] = raw(b"\x01" + bytes(8))
    cases.append(("a 9-byte Number and a 9-byte GasLimit", _list(g), BAD))
    return cases


# ---------------------------------------------------------------- headers behind a parent
def child(cfg, parent, parent_blob, dt=10, salt=0, **over):
    """a valid child of `parent` (dict; its encoding parent_blob), then the overrides.  Difficulty follows the
    (possibly overridden) Time unless it is overridden itself."""
    h = B.new_header(ParentHash=B.header_hash(parent_blob), Coinbase=bytes([salt & 0xFF]) * 20,
                     Root=bytes([(salt >> 8) & 0xFF]) * 32, Number=(parent["Number"] + 1) & U64, Time=parent["Time"] + dt,
                     GasLimit=parent["GasLimit"], GasUsed=0, Extra=b"case", MixDigest=bytes([0x5A]) * 32,
                     Nonce=bytes([0xA5]) * 8)
    fix = {k: v for k, v in over.items() if k != "Difficulty"}
    h.update(fix)
    h["Difficulty"] = over["Difficulty"] if "Difficulty" in over else \
        min(B.calc_difficulty(cfg, h["Time"] & U64, parent), (1 << 256) - 1)
    return h


def rule_cases(parent, now):
    """(name, overrides of the middle header, its status) for segments [good, X, child of X] under TEST_CONFIG:
    each check failing alone, then pairs that show the order.  `parent` is the segment's parent: X's own parent
    `good` has its GasLimit and the next Number."""
    lim = parent["GasLimit"] // 1024
    gl = parent["GasLimit"]
    return [
        ("valid", {}, B.ST_OK),
        ("Extra of 32 bytes", {"Extra": bytes(32)}, B.ST_OK),
        ("Extra of 33 bytes", {"Extra": bytes(33)}, B.ST_EXTRA_TOO_LONG),
        ("Extra of 70 bytes", {"Extra": bytes(70)}, B.ST_EXTRA_TOO_LONG),
        ("Time at now + 15", {"Time": now + 15}, B.ST_OK),
        ("Time at now + 16", {"Time": now + 16}, B.ST_FUTURE_BLOCK),
        ("Time of 2^64", {"Time": 1 << 64}, B.ST_FUTURE_BLOCK),
        ("Time of 2^255", {"Time": 1 << 255}, B.ST_FUTURE_BLOCK),
        ("Time equal to the parent's", {"dt": 0}, B.ST_ZERO_BLOCK_TIME),
        ("Time before the parent's", {"dt": -1}, B.ST_ZERO_BLOCK_TIME),
        ("Difficulty one above", {"Difficulty": +1}, B.ST_WRONG_DIFFICULTY),
        ("Difficulty one below", {"Difficulty": -1}, B.ST_WRONG_DIFFICULTY),
        ("Difficulty of zero", {"Difficulty": 0}, B.ST_WRONG_DIFFICULTY),
        ("GasLimit of 2^63", {"GasLimit": 1 << 63}, B.ST_GAS_LIMIT_CAP),
        ("GasLimit of 2^64 - 1", {"GasLimit": U64}, B.ST_GAS_LIMIT_CAP),
        ("GasLimit of 2^63 - 1", {"GasLimit": (1 << 63) - 1}, B.ST_GAS_LIMIT_BOUNDS),
        ("GasUsed at the limit", {"GasUsed": gl}, B.ST_OK),
        ("GasUsed one above the limit", {"GasUsed": gl + 1}, B.ST_GAS_USED),
        ("GasLimit up by the bound less one", {"GasLimit": gl + lim - 1}, B.ST_OK),
        ("GasLimit up by the bound", {"GasLimit": gl + lim}, B.ST_GAS_LIMIT_BOUNDS),
        ("GasLimit up by the bound and one", {"GasLimit": gl + lim + 1}, B.ST_GAS_LIMIT_BOUNDS),
        ("GasLimit down by the bound less one", {"GasLimit": gl - lim + 1}, B.ST_OK),
        ("GasLimit down by the bound", {"GasLimit": gl - lim}, B.ST_GAS_LIMIT_BOUNDS),
        ("Number two above", {"Number": parent["Number"] + 3}, B.ST_INVALID_NUMBER),
        ("Number equal to its parent's", {"Number": parent["Number"] + 1}, B.ST_INVALID_NUMBER),
        ("Number of zero", {"Number": 0}, B.ST_INVALID_NUMBER),
        # pairs: the earlier check is the status
        ("Extra too long and in the future", {"Extra": bytes(33), "Time": now + 16}, B.ST_EXTRA_TOO_LONG),
        ("in the future and a wrong difficulty", {"Time": now + 16, "Difficulty": 0}, B.ST_FUTURE_BLOCK),
        ("a zero block time and a wrong difficulty", {"dt": 0, "Difficulty": 0}, B.ST_ZERO_BLOCK_TIME),
        ("a wrong difficulty and the gas cap", {"Difficulty": +1, "GasLimit": 1 << 63}, B.ST_WRONG_DIFFICULTY),
        ("the gas cap and gas used", {"GasLimit": 1 << 63, "GasUsed": U64}, B.ST_GAS_LIMIT_CAP),
        ("gas used and the gas bounds", {"GasLimit": gl + lim, "GasUsed": gl + lim + 1}, B.ST_GAS_USED),
        ("the gas bounds and the number", {"GasLimit": gl + lim, "Number": 0}, B.ST_GAS_LIMIT_BOUNDS),
    ]


def rule_segment(parent, parent_blob, over, salt):
    """[good, X, child of X] as (blobs, index of X): `over` as in rule_cases, Difficulty there an offset to the
    expected value (0: the value zero), dt the step from X's parent"""
    cfg = TEST_CONFIG
    good = child(cfg, parent, parent_blob, salt=salt)
    gb = B.encode_header(good)
    o = dict(over)
    dt = o.pop("dt", 10)
    off = o.pop("Difficulty", None)
    x = child(cfg, good, gb, dt=dt, salt=salt + 1, **o)
    if off is not None:
        x["Difficulty"] = 0 if off == 0 else x["Difficulty"] + off
    xb = B.encode_header(x)
    last = child(cfg, x, xb, salt=salt + 2)
    return [gb, xb, B.encode_header(last)], 1


# ---------------------------------------------------------------- CalcDifficulty
DELTAS = (1, 8, 9, 10, 12, 13, 17, 18, 899, 900, 10 ** 6)
PARENT_DIFFICULTIES = (131072, 131073, 1 << 64, 1 << 255)


def difficulty_cases():
    """(config, time, parent header) over the three rule sets"""
    frontier = B.Config()
    homestead = B.Config(homestead=0)
    byzantium = B.Config(homestead=0, byzantium=0)
    forks = B.Config(homestead=1150000, byzantium=4370000)
    out = []
    t0 = 1500000000
    for cfg in (frontier, homestead, byzantium):
        for dt in DELTAS:
            for uncle in (B.EMPTY_UNCLE_HASH, bytes(32)):
                for pd in PARENT_DIFFICULTIES:
                    out.append((cfg, t0 + dt, B.new_header(Difficulty=pd, Number=50, Time=t0, UncleHash=uncle)))
    # the bomb: periods 0, 1, 2, 3, the last one below 2^256 and the first ones past it
    for cfg in (frontier, homestead):
        for number in (99998, 99999, 199998, 199999, 299999, 25699999, 25799998, 25799999, 25800000, 1 << 40, U64 - 1, U64):
            for pd in (131072, 1 << 255):
                out.append((cfg, t0 + 20, B.new_header(Difficulty=pd, Number=number, Time=t0)))
    for number in (0, 2999998, 2999999, 3099999, 3199998, 3199999, 3200000, 3299999, 2999999 + 25800000 - 1,
                   2999999 + 25800000, U64 - 1, U64):
        for pd in (131072, (1 << 255) + 12345):
            out.append((byzantium, t0 + 5, B.new_header(Difficulty=pd, Number=number, Time=t0)))
    # the fork edges: parent.Number + 1 == fork
    for number in (1149998, 1149999, 1150000, 4369998, 4369999, 4370000):
        for dt in (5, 9, 10, 13, 100):
            out.append((forks, t0 + dt, B.new_header(Difficulty=1 << 50, Number=number, Time=t0, UncleHash=bytes(32))))
    # a time before the parent's (the bare CalcDifficulty only): big.Int.Div floors
    for cfg in (frontier, homestead, byzantium):
        for back in (1, 9, 10, 11, 12345):
            out.append((cfg, t0 - back, B.new_header(Difficulty=1 << 30, Number=50, Time=t0)))
        out.append((cfg, 5, B.new_header(Difficulty=1 << 30, Number=50, Time=1 << 200)))
        out.append((cfg, 5, B.new_header(Difficulty=1 << 250, Number=50, Time=(1 << 256) - 1)))
        out.append((cfg, U64, B.new_header(Difficulty=1 << 30, Number=50, Time=1 << 64)))
    return out


# ---------------------------------------------------------------- gas
def gas_cases():
    """(parent GasLimit, GasLimit, GasUsed, status of a header otherwise valid)"""
    OK, CAP, USED, BOUNDS = B.ST_OK, B.ST_GAS_LIMIT_CAP, B.ST_GAS_USED, B.ST_GAS_LIMIT_BOUNDS
    top = (1 << 63) - 1
    return [(5000, 5000, 0, OK), (5000, 4999, 0, BOUNDS), (5000, 5003, 5003, OK), (5000, 5004, 0, BOUNDS),
            (5120, 5000, 0, BOUNDS), (5121, 5000, 0, BOUNDS), (6000, 5000, 0, BOUNDS), (5004, 5000, 0, BOUNDS),
            (5003, 5000, 5000, OK), (1024, 1024, 0, BOUNDS), (0, 0, 0, BOUNDS), (1023, 5000, 0, BOUNDS),
            (1 << 20, (1 << 20) + 1023, 0, OK), (1 << 20, (1 << 20) + 1024, 0, BOUNDS),
            (1 << 20, (1 << 20) - 1023, 0, OK), (1 << 20, (1 << 20) - 1024, 0, BOUNDS),
            (top, top, top, OK), (top, 1 << 63, 0, CAP), (top, top, top + 1, USED),
            # a parent above 2^63: int64() wraps it negative, and the difference wraps again
            ((1 << 63) + 5, top, 0, OK), ((1 << 63) + 5, 5000, 0, BOUNDS), (U64, top, 0, BOUNDS),
            (U64, 5000, 0, OK), (1 << 63, top, 0, OK), (1 << 63, 1 << 62, 0, BOUNDS)]
