"""Inputs shared by the blob codec's CPU and GPU tests (tests/test_blob_codec_host.py,
tests/test_gpu_blob_codec.py): lists of (blob, skip_evm) and bodies with the decoder's edge cases."""
import random

# the kernel's launch constants (csrc/blob.hip): a lane stores 16 bytes, a wave 1,024, a workgroup 4,096
BS_GROUP_BYTES, BS_WAVE_BYTES, BS_BLOCK_BYTES = 16, 1024, 4096


def _blob(rng, n):
    # no zero bytes, no 0xFF: a filler byte or a byte of the 0xFF surroundings that leaks shows
    return bytes(rng.randrange(1, 255) for _ in range(n))


def length_corpus():
    """one list: every length 0..130 with both flag values, then 31k - 1, 31k, 31k + 1 for k in
    {64, 256, 2048}"""
    rng = random.Random(31)
    out = []
    for n in range(131):
        for f in (0, 1):
            out.append((_blob(rng, n), f))
    for k in (64, 256, 2048):
        for d in (-1, 0, 1):
            out.append((_blob(rng, 31 * k + d), (k + d) & 1))
    return out


def marshal_test_vector():
    """sharding/utils/marshal_test.go:183-217 TestSerializeTestData: 60 bytes 0..59"""
    return [(bytes(range(60)), 0)]


def list_sets():
    """batches of 1, 2 and 5 lists with unequal blob counts; a list of one 1-byte blob and an empty
    list between full ones; lists holding zero-length blobs"""
    rng = random.Random(7)
    full = length_corpus()
    a = [(_blob(rng, n), n & 1) for n in (1, 31, 32, 62, 0, 93, 5, 0, 0, 200)]
    b = [(_blob(rng, n), 0) for n in (0, 0, 17)]
    one = [(b"\x07", 1)]
    return {
        "one list": [full],
        "two lists": [a, full[:40]],
        "five lists": [full[:64], one, [], a, b],
        "only empty blobs": [[(b"", 0), (b"", 1)], []],
        "no blobs": [[]],
        "marshal_test": [marshal_test_vector()],
    }


def straddle_lists():
    """a list whose blobs cross every 16-byte group, 1,024-byte wave and 4,096-byte workgroup
    boundary of the output up to 3 workgroups: blobs of 124 bytes (4 chunks = 128 output bytes) shifted by
    one leading blob of every size class, and one long blob over several workgroups"""
    rng = random.Random(11)
    out = []
    for lead in (1, 31, 32, 63, 94):  # 1, 1, 2, 3, 4 chunks: moves every later boundary by 32..128 bytes
        lst = [(_blob(rng, lead), 0)]
        total = 32 * ((lead + 30) // 31)
        while total < 3 * BS_BLOCK_BYTES:
            n = rng.choice((124, 100, 45, 310))
            lst.append((_blob(rng, n), rng.randrange(2)))
            total += 32 * ((n + 30) // 31)
        out.append(lst)
    out.append([(_blob(rng, 5), 1), (_blob(rng, 31 * 300 + 9), 0), (_blob(rng, 40), 1)])  # 9.6 KB of output
    return out


def edge_bodies():
    """bodies for Deserialize: the notary test's edge cases and a body ending in non-terminal chunks"""
    rng = random.Random(13)

    def chunk(ind, data=None):
        return bytes([ind]) + (data if data is not None else _blob(rng, 31))

    plain = b"".join([chunk(0), chunk(5), chunk(31), chunk(0), chunk(0), chunk(0x80 | 1)])
    return {
        "plain": plain,
        "trailing partial chunk": plain + b"\x05" + _blob(rng, 17),
        "indicator bits 0x60 set": b"".join([chunk(0x60), chunk(0x60 | 9), chunk(0x40), chunk(0xE0 | 31), chunk(0x20 | 2)]),
        "ends in non-terminal chunks": plain + chunk(0) + chunk(0x60) + chunk(0),
        "no terminal chunk": chunk(0) + chunk(0),
        "less than a chunk": b"\x03abc",
        "empty": b"",
        "blobs that are no transactions": b"".join(chunk(1 + (i % 31)) for i in range(70)),
    }
