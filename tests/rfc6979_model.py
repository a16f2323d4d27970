"""RFC 6979's nonce as crypto.Sign gets it (libsecp256k1's nonce_function_rfc6979 with no extra data and
no algorithm tag: libsecp256k1/src/secp256k1.c:310-340 over src/hash_impl.h:205-264), in Python over
hmac / hashlib.  The model of csrc/rfc6979_dev.cuh for the CPU tests, and the only place besides the host
build of that header where a counter past 0 can be reached.

    V = 01 x 32, K = 00 x 32
    K = HMAC(K, V || 00 || key || msg), V = HMAC(K, V)
    K = HMAC(K, V || 01 || key || msg), V = HMAC(K, V)
    output c: for every output after the first K = HMAC(K, V || 00), V = HMAC(K, V); then V = HMAC(K, V)
"""
import hashlib
import hmac

N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


def _h(k, m):
    return hmac.new(k, m, hashlib.sha256).digest()


def nonce(key: bytes, msg: bytes, counter: int = 0) -> bytes:
    """key, msg: 32 bytes each (msg raw, not reduced); the generator's output number `counter`"""
    assert len(key) == 32 and len(msg) == 32
    v, k = b"\x01" * 32, b"\x00" * 32
    k = _h(k, v + b"\x00" + key + msg)
    v = _h(k, v)
    k = _h(k, v + b"\x01" + key + msg)
    v = _h(k, v)
    for c in range(counter + 1):
        if c:
            k = _h(k, v + b"\x00")
            v = _h(k, v)
        v = _h(k, v)
    return v


def edge_pairs():
    """(key, msg) pairs at the ends of both ranges: keys 1 and n - 1, messages 0, n - 1, n, n + 1, 2^256 - 1"""
    keys = [1, N - 1, 2, N // 2, N // 2 + 1]
    msgs = [0, N - 1, N, N + 1, 2**256 - 1, 1]
    return [(k.to_bytes(32, "big"), m.to_bytes(32, "big")) for k in keys for m in msgs]


def random_pairs(count, seed):
    import random
    rng = random.Random(seed)
    return [(rng.randrange(1, N).to_bytes(32, "big"), rng.getrandbits(256).to_bytes(32, "big")) for _ in range(count)]
