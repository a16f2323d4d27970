"""ecies.Encrypt / PrivateKey.Decrypt for ECIES_AES128_SHA256 with s1 empty, in plain Python: the
semantics gsv_ecies_decrypt_batch and gsv_ecies_encrypt_batch pin (include/gsv.h), restated from
crypto/ecies/ecies.go:246-366.  AES-128 is written out from FIPS-197 (the S-box computed from its
definition, section 5.1.1), CTR mode is Go's cipher.NewCTR (the whole 16-byte block one big-endian
counter), the tag is hmac / hashlib's, the curve code is secp_ecdh_model's.

Also the rows the fixture (tests/golden/make_ecies.py) and the GPU tests share.
"""
import functools
import hashlib
import hmac
import random

import secp_ecdh_model as E

ST_OK, ST_INVALID_PUBKEY, ST_INVALID_KEY, ST_INVALID_CURVE, ST_INVALID_MESSAGE = 0, 7, 11, 12, 14
OVERHEAD = 113  # 65 (R) + 16 (IV) + 32 (tag): eciesOverhead, p2p/rlpx.go:58


# ---------------------------------------------------------------- AES-128 (FIPS-197)
def _xtime(a):
    a <<= 1
    return (a ^ 0x11B) & 0xFF if a & 0x100 else a


def _gmul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a = _xtime(a)
        b >>= 1
    return r


def _make_sbox():
    """5.1.1: the multiplicative inverse in GF(2^8) (0 -> 0), then the affine transformation"""
    inv = [0] * 256
    for a in range(1, 256):
        for b in range(1, 256):
            if _gmul(a, b) == 1:
                inv[a] = b
                break
    box = []
    for a in range(256):
        x = inv[a]
        y = x
        for k in range(1, 5):
            y ^= ((x << k) | (x >> (8 - k))) & 0xFF
        box.append(y ^ 0x63)
    return box


SBOX = _make_sbox()
assert SBOX[0] == 0x63 and SBOX[0x53] == 0xED and SBOX[0xFF] == 0x16


def aes128_expand(key: bytes):
    """5.2 KeyExpansion: 44 words as 4-byte lists"""
    assert len(key) == 16
    w = [list(key[4 * i:4 * i + 4]) for i in range(4)]
    rcon = 1
    for i in range(4, 44):
        t = list(w[i - 1])
        if i % 4 == 0:
            t = [SBOX[b] for b in t[1:] + t[:1]]
            t[0] ^= rcon
            rcon = _xtime(rcon)
        w.append([a ^ b for a, b in zip(w[i - 4], t)])
    return w


def aes128_encrypt_block(w, block: bytes) -> bytes:
    """5.1 Cipher; the state is column-major: s[r][c] = in[r + 4c]"""
    s = list(block)

    def add(rnd):
        for c in range(4):
            for r in range(4):
                s[r + 4 * c] ^= w[4 * rnd + c][r]

    add(0)
    for rnd in range(1, 11):
        t = [SBOX[b] for b in s]
        t = [t[r + 4 * ((c + r) % 4)] for c in range(4) for r in range(4)]  # ShiftRows
        if rnd < 10:
            m = []
            for c in range(4):
                a = t[4 * c:4 * c + 4]
                m += [_gmul(a[0], 2) ^ _gmul(a[1], 3) ^ a[2] ^ a[3], a[0] ^ _gmul(a[1], 2) ^ _gmul(a[2], 3) ^ a[3],
                      a[0] ^ a[1] ^ _gmul(a[2], 2) ^ _gmul(a[3], 3), _gmul(a[0], 3) ^ a[1] ^ a[2] ^ _gmul(a[3], 2)]
            t = m
        s[:] = t
        add(rnd)
    return bytes(s)


def aes128_ctr(key: bytes, iv: bytes, data: bytes) -> bytes:
    """cipher.NewCTR(aes, iv).XORKeyStream: the counter block is one 128-bit big-endian integer"""
    assert len(iv) == 16
    w = aes128_expand(key)
    ctr = int.from_bytes(iv, "big")
    out = bytearray()
    for o in range(0, len(data), 16):
        ks = aes128_encrypt_block(w, ctr.to_bytes(16, "big"))
        out += bytes(a ^ b for a, b in zip(data[o:o + 16], ks))
        ctr = (ctr + 1) % (1 << 128)
    return bytes(out)


def message_tag(km: bytes, em: bytes, s2: bytes) -> bytes:
    return hmac.new(km, em + s2, hashlib.sha256).digest()


# ---------------------------------------------------------------- the rules
@functools.lru_cache(maxsize=None)
def _ecdh(pub64: bytes, seckey32: bytes):
    """secp_ecdh_model.ecdh, remembered: batches of test items share a few key pairs"""
    return E.ecdh(pub64, seckey32)


@functools.lru_cache(maxsize=None)
def _pub_of(seckey32: bytes) -> bytes:
    return E.pt64(E.ec_mul(int.from_bytes(seckey32, "big"), E.G))


def decrypt(c: bytes, seckey32: bytes, s2: bytes = b""):
    """gsv_ecies_decrypt_batch for one item: (status, message).  The checks in the reference's order;
    the first failure decides."""
    assert len(seckey32) == 32
    if len(c) == 0:
        return ST_INVALID_MESSAGE, b""
    if c[0] not in (2, 3, 4):
        return ST_INVALID_PUBKEY, b""
    if len(c) < 98:
        return ST_INVALID_MESSAGE, b""
    if c[0] != 4:  # rLen is 65 for all three; elliptic.Unmarshal takes only 04
        return ST_INVALID_PUBKEY, b""
    x, y = int.from_bytes(c[1:33], "big"), int.from_bytes(c[33:65], "big")
    if x >= E.P or y >= E.P:  # the strict reading (include/gsv.h)
        return ST_INVALID_PUBKEY, b""
    if not E.on_curve(x, y):
        return ST_INVALID_CURVE, b""
    k = int.from_bytes(seckey32, "big")
    if k == 0 or k >= E.N:
        return ST_INVALID_KEY, b""
    if len(c) < OVERHEAD:  # em shorter than an IV
        return ST_INVALID_MESSAGE, b""
    st, _, keys = _ecdh(c[1:65], seckey32)
    assert st == ST_OK
    ke, km = keys[:16], keys[16:]
    em, tag = c[65:-32], c[-32:]
    if not hmac.compare_digest(tag, message_tag(km, em, s2)):
        return ST_INVALID_MESSAGE, b""
    return ST_OK, aes128_ctr(ke, em[:16], em[16:])


def encrypt(m: bytes, pub64: bytes, eph32: bytes, iv: bytes, s2: bytes = b""):
    """gsv_ecies_encrypt_batch for one item: (status, 113 + len(m) bytes; zeros when it failed)"""
    assert len(pub64) == 64 and len(eph32) == 32 and len(iv) == 16
    zero = bytes(OVERHEAD + len(m))
    st, _, keys = _ecdh(pub64, eph32)  # the key rule first, then the curve rule
    if st != ST_OK:
        return st, zero
    if len(m) == 0:
        return ST_INVALID_MESSAGE, zero
    ke, km = keys[:16], keys[16:]
    em = iv + aes128_ctr(ke, iv, m)
    return ST_OK, b"\x04" + _pub_of(eph32) + em + message_tag(km, em, s2)


def keys_of(pub64: bytes, seckey32: bytes):
    """(Ke, Km) of a valid pair"""
    st, _, keys = _ecdh(pub64, seckey32)
    assert st == ST_OK
    return keys[:16], keys[16:]


# ---------------------------------------------------------------- the shared rows
MSG_LENS = (0, 1, 15, 16, 17, 38, 39, 40, 47, 48, 49, 97, 102, 103, 104, 194, 1000)
S2_LENS = (0, 2, 7, 64)
CARRY_IVS = (b"\xff" * 16, bytes(12) + b"\xff" * 4, bytes(8) + b"\xff" * 8)
SEED = 0xEC1E5


def _rand_bytes(rng, n):
    return bytes(rng.randrange(256) for _ in range(n))


def _pair(rng):
    """(secret key bytes, public point 64 bytes)"""
    k = E.be32(rng.randrange(1, E.N))
    return k, _pub_of(k)


def good_rows():
    """[(tag, msg, pub64 of the recipient, seckey32 of the recipient, eph32, iv, s2)]: every message length
    with every s2 length cycling, every s2 length at three message lengths, the carry IVs.  Two recipients
    and four ephemeral keys are shared by all rows: the model's multiplications are the slow part."""
    rng = random.Random(SEED)
    rcpt = [_pair(rng) for _ in range(2)]
    ephs = [_pair(rng)[0] for _ in range(4)]
    rows = []

    def add(tag, mlen, s2len, iv=None):
        j = len(rows)
        sk, pub = rcpt[j % 2]
        rows.append((tag, _rand_bytes(rng, mlen), pub, sk, ephs[j % 4], iv or _rand_bytes(rng, 16),
                     _rand_bytes(rng, s2len)))

    for j, mlen in enumerate(MSG_LENS):
        add("len", mlen, S2_LENS[j % 4])
    for mlen in (1, 39, 103):
        for s2len in S2_LENS:
            add("s2", mlen, s2len)
    for iv in CARRY_IVS:
        add("carry", 33, 0, iv)
        add("carry", 70, 2, iv)
    return rows


def bad_rows():
    """[(tag, ciphertext, seckey32, s2, expected status)]: one row at least for every numbered failure of
    Decrypt, built from a good ciphertext"""
    rng = random.Random(SEED + 1)
    sk, pub = _pair(rng)
    eph = _pair(rng)[0]
    s2 = b"\x01\x42"
    st, good = encrypt(_rand_bytes(rng, 50), pub, eph, _rand_bytes(rng, 16), s2)
    assert st == ST_OK
    rows = []

    def add(tag, c, want, key=sk, s=s2):
        rows.append((tag, bytes(c), key, s, want))

    def flip(pos, bit=1):
        c = bytearray(good)
        c[pos] ^= bit
        return c

    add("1 empty", b"", ST_INVALID_MESSAGE)
    add("2 first byte 00", flip(0, 4), ST_INVALID_PUBKEY)
    add("2 first byte 05, one byte long", b"\x05", ST_INVALID_PUBKEY)
    add("3 len 97", good[:97], ST_INVALID_MESSAGE)
    add("3 first byte 02, len 97", b"\x02" + good[1:97], ST_INVALID_MESSAGE)
    add("4 first byte 02", b"\x02" + good[1:], ST_INVALID_PUBKEY)
    add("4 first byte 03", b"\x03" + good[1:], ST_INVALID_PUBKEY)
    t = E.point_x1()
    add("5 x + p", b"\x04" + E.be32(t[0] + E.P) + E.be32(t[1]) + good[65:], ST_INVALID_PUBKEY)
    add("5 y = p", b"\x04" + good[1:33] + E.be32(E.P) + good[65:], ST_INVALID_PUBKEY)
    add("6 off curve", flip(64), ST_INVALID_CURVE)
    add("6 off curve, bad key", flip(64), ST_INVALID_CURVE, key=bytes(32))
    add("7 key 0", good, ST_INVALID_KEY, key=bytes(32))
    add("7 key n", good, ST_INVALID_KEY, key=E.be32(E.N))
    add("7 key 0, len 98", good[:98], ST_INVALID_KEY, key=bytes(32))
    add("8 len 98", good[:98], ST_INVALID_MESSAGE)
    add("8 len 112", good[:112], ST_INVALID_MESSAGE)
    add("9 first tag byte", flip(len(good) - 32, 0x80), ST_INVALID_MESSAGE)
    add("9 last tag byte", flip(len(good) - 1), ST_INVALID_MESSAGE)
    add("9 ciphertext bit", flip(90, 0x10), ST_INVALID_MESSAGE)
    add("9 iv bit", flip(65), ST_INVALID_MESSAGE)
    add("9 wrong s2", good, ST_INVALID_MESSAGE, s=b"\x01\x43")
    add("9 s2 missing", good, ST_INVALID_MESSAGE, s=b"")
    add("9 another key", good, ST_INVALID_MESSAGE, key=eph)
    # len 113: a valid empty message (Encrypt never makes one, so the tag is made here)
    ke, km = keys_of(pub, eph)
    R = good[:65]
    iv = _rand_bytes(rng, 16)
    add("10 len 113", R + iv + message_tag(km, iv, s2), ST_OK)
    add("9 len 113, wrong tag", R + iv + message_tag(km, iv, b""), ST_INVALID_MESSAGE)
    add("10 good", good, ST_OK)
    return rows


def batch_items(count, seed=SEED + 2):
    """[(msg, pub64, seckey32, eph32, iv, s2, ct)] for the launch-shape tests: seeded messages of mixed
    lengths from MSG_LENS (0 and 1000 side by side at items 2 and 3), s2 of mixed lengths, two recipients and
    four ephemeral keys.  ct opens to msg under seckey32; for the empty message, which Encrypt refuses, it is
    the 113 bytes Decrypt accepts."""
    rng = random.Random(seed)
    rcpt = [_pair(rng) for _ in range(2)]
    ephs = [_pair(rng)[0] for _ in range(4)]
    items = []
    for j in range(count):
        mlen = {2: 0, 3: 1000}.get(j, MSG_LENS[rng.randrange(len(MSG_LENS) - 1)])  # 1000 only once: the model is slow
        sk, pub = rcpt[rng.randrange(2)]
        eph = ephs[rng.randrange(4)]
        msg, iv, s2 = _rand_bytes(rng, mlen), _rand_bytes(rng, 16), _rand_bytes(rng, S2_LENS[rng.randrange(4)])
        if mlen:
            st, ct = encrypt(msg, pub, eph, iv, s2)
            assert st == ST_OK
        else:
            ct = b"\x04" + _pub_of(eph) + iv + message_tag(keys_of(pub, eph)[1], iv, s2)
        items.append((msg, pub, sk, eph, iv, s2, ct))
    return items
