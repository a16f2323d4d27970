"""A numpy model of consensus/ethash written from algorithm.go, vectorised across the batch: Keccak-f runs
on [n, 25] uint64 arrays and the 256-parent loop of generateDatasetItem on [n, 16] uint32 arrays.

    generate_cache(size, seed)                  algorithm.go:128-197 (row by row: small sizes only)
    dataset_item(cache_words, indices)          algorithm.go:232-261
    hashimoto_light(size, cache_words, hashes, nonces)   algorithm.go:375
    hashimoto_full(size, dataset_words, hashes, nonces)  algorithm.go:391

cache_words / dataset_words: uint32 arrays of shape [rows, 16] (the little-endian words of the bytes).
"""
import numpy as np

FNV_PRIME = np.uint32(0x01000193)
_RC = np.array([
    0x0000000000000001, 0x0000000000008082, 0x800000000000808A, 0x8000000080008000, 0x000000000000808B,
    0x0000000080000001, 0x8000000080008081, 0x8000000000008009, 0x000000000000008A, 0x0000000000000088,
    0x0000000080008009, 0x000000008000000A, 0x000000008000808B, 0x800000000000008B, 0x8000000000008089,
    0x8000000000008003, 0x8000000000008002, 0x8000000000000080, 0x000000000000800A, 0x800000008000000A,
    0x8000000080008081, 0x8000000000008080, 0x0000000080000001, 0x8000000080008008], dtype=np.uint64)
_RHO = [0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14]


def _rotl(v, r):
    if r == 0:
        return v
    return (v << np.uint64(r)) | (v >> np.uint64(64 - r))


def keccak_f(a):
    """Keccak-f[1600] over a [n, 25] uint64 array (crypto/sha3/keccakf.go), returns a new array"""
    a = a.copy()
    for rnd in range(24):
        c = a[:, 0:5] ^ a[:, 5:10] ^ a[:, 10:15] ^ a[:, 15:20] ^ a[:, 20:25]
        d = np.roll(c, 1, axis=1) ^ _rotl(np.roll(c, -1, axis=1), 1)
        a ^= np.tile(d, (1, 5))
        b = np.empty_like(a)
        for x in range(5):
            for y in range(5):
                b[:, y + 5 * ((2 * x + 3 * y) % 5)] = _rotl(a[:, x + 5 * y], _RHO[x + 5 * y])
        for y in range(0, 25, 5):
            row = b[:, y:y + 5]
            a[:, y:y + 5] = row ^ (~np.roll(row, -1, axis=1) & np.roll(row, -2, axis=1))
        a[:, 0] ^= _RC[rnd]
    return a


def keccak(data, out_len):
    """pre-FIPS Keccak (pad 0x01 ... 0x80) of every row of data [n, len] uint8, one block: len < rate.
    Returns [n, out_len] uint8."""
    data = np.ascontiguousarray(data, np.uint8)
    n, ln = data.shape
    rate = 200 - 2 * out_len
    assert ln < rate
    block = np.zeros((n, 200), np.uint8)
    block[:, :ln] = data
    block[:, ln] ^= 0x01
    block[:, rate - 1] ^= 0x80
    st = keccak_f(block.view("<u8").reshape(n, 25))
    return np.ascontiguousarray(st[:, :out_len // 8]).view(np.uint8).reshape(n, out_len)


def keccak512(data):
    return keccak(data, 64)


def keccak256(data):
    return keccak(data, 32)


def keccak256_bytes(b):
    """Keccak-256 of one byte string of any length -> 32 bytes"""
    raw = np.frombuffer(bytes(b), np.uint8)
    padded = np.concatenate([raw, np.zeros(136 - len(raw) % 136, np.uint8)])
    padded[len(raw)] ^= 0x01
    padded[-1] ^= 0x80
    st = np.zeros((1, 25), np.uint64)
    for at in range(0, len(padded), 136):
        st[0, :17] ^= padded[at:at + 136].view("<u8")
        st = keccak_f(st)
    return np.ascontiguousarray(st[0, :4]).view(np.uint8).tobytes()


def item_bytes(items):
    """[n, 16] uint32 items -> their bytes"""
    return np.ascontiguousarray(np.asarray(items).astype("<u4")).view(np.uint8).reshape(-1).tobytes()


def words(b):
    """bytes or uint8 array -> [rows, 16] little-endian uint32"""
    return np.frombuffer(bytes(b), "<u4").reshape(-1, 16).astype(np.uint32)


def generate_cache(size, seed):
    """the cache's bytes (uint8 [size]); a Python loop over rows, for small sizes"""
    rows = size // 64
    out = np.zeros((rows, 64), np.uint8)
    out[0] = keccak512(np.frombuffer(bytes(seed), np.uint8).reshape(1, 32))[0]
    for r in range(1, rows):
        out[r] = keccak512(out[r - 1:r])[0]
    for _ in range(3):
        for j in range(rows):
            x = int(out[j, :4].view("<u4")[0]) % rows
            out[j] = keccak512((out[(j - 1 + rows) % rows] ^ out[x]).reshape(1, 64))[0]
    return out.reshape(-1)


def _fnv(a, b):
    return (a * FNV_PRIME) ^ b


def dataset_item(cache_words, indices):
    """generateDatasetItem for every index: [n, 16] uint32"""
    cache_words = np.asarray(cache_words, np.uint32)
    idx = np.asarray(indices, np.uint32).reshape(-1)
    rows = np.uint32(cache_words.shape[0])
    mix = cache_words[idx % rows].copy()
    mix[:, 0] ^= idx
    mix = np.ascontiguousarray(keccak512(np.ascontiguousarray(mix).view(np.uint8).reshape(-1, 64))).view("<u4").astype(
        np.uint32)
    for i in range(256):
        parent = _fnv(idx ^ np.uint32(i), mix[:, i % 16]) % rows
        mix = _fnv(mix, cache_words[parent])
    return np.ascontiguousarray(keccak512(np.ascontiguousarray(mix).view(np.uint8).reshape(-1, 64))).view("<u4").astype(
        np.uint32)


def _hashimoto(size, hashes, nonces, lookup):
    h = np.ascontiguousarray(hashes, np.uint8).reshape(-1, 32)
    n = h.shape[0]
    nn = np.ascontiguousarray(np.asarray(nonces, np.uint64).reshape(n, 1)).view(np.uint8).reshape(n, 8)
    rows = np.uint32(size // 128)
    seed = keccak512(np.concatenate([h, nn], axis=1))
    sw = np.ascontiguousarray(seed).view("<u4").astype(np.uint32)
    head = sw[:, 0]
    mix = np.tile(sw, (1, 2))
    for i in range(64):
        parent = _fnv(np.uint32(i) ^ head, mix[:, i % 32]) % rows
        temp = np.concatenate([lookup(np.uint32(2) * parent), lookup(np.uint32(2) * parent + np.uint32(1))], axis=1)
        mix = _fnv(mix, temp)
    m = mix.reshape(n, 8, 4)
    digest = _fnv(_fnv(_fnv(m[:, :, 0], m[:, :, 1]), m[:, :, 2]), m[:, :, 3])
    digest = np.ascontiguousarray(digest.astype("<u4")).view(np.uint8).reshape(n, 32)
    return digest, keccak256(np.concatenate([seed, digest], axis=1))


def hashimoto_light(size, cache_words, hashes, nonces):
    """(digests [n, 32], results [n, 32]) uint8"""
    return _hashimoto(size, hashes, nonces, lambda idx: dataset_item(cache_words, idx))


def hashimoto_full(size, dataset_words, hashes, nonces):
    dataset_words = np.asarray(dataset_words, np.uint32)
    return _hashimoto(size, hashes, nonces, lambda idx: dataset_words[idx])
