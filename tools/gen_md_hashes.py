"""Generates tests/golden/md_hashes.json: RIPEMD-160 digests for tests/ripemd160_model.py and the GPU tests.

"spec": the nine test vectors published with the RIPEMD-160 specification (the 10^6 x "a" message is
stored as {"repeat": "a", "count": 1000000}).  "random": the model's digests of seeded messages of lengths
0 - 300 and of the 100,000-byte ripemd160_model.long_message.  Every digest is cross-checked against `openssl dgst -provider legacy
-ripemd160` before anything is written; without an openssl that has the legacy provider the script
refuses to write.  The tests read only the fixture.

    python tools/gen_md_hashes.py
"""
import json
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ripemd160_model as M  # noqa: E402

SPEC = [
    (b"", "9c1185a5c5e9fc54612808977ee8f548b2258d31"),
    (b"a", "0bdc9d2d256b3ee9daae347be6f4dc835a467ffe"),
    (b"abc", "8eb208f7e05d987a9b044a8e98c6b087f15a0bfc"),
    (b"message digest", "5d0689ef49d2fae572b881b123a85ffa21595f36"),
    (b"abcdefghijklmnopqrstuvwxyz", None),
    (b"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq", "12a053384a9c0c88e405a06c27dcf49ada62eb2b"),
    (b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789", None),
    (b"1234567890" * 8, "9b752e45573d4b39f4dbd3323cab82bf63326bfb"),
    (b"a" * 1000000, "52783243c1697bdbe16d37f97f68f08325dc1528"),
]
LENS = [0, 1, 2, 3, 4, 5, 31, 32, 33, 54, 55, 56, 57, 62, 63, 64, 65, 66, 100, 111, 118, 119, 120, 121, 126, 127,
        128, 129, 160, 183, 184, 191, 192, 193, 200, 247, 248, 255, 256, 300]


def openssl(msg: bytes) -> str:
    r = subprocess.run(["openssl", "dgst", "-provider", "legacy", "-provider", "default", "-ripemd160", "-r"],
                       input=msg, capture_output=True, check=True)
    return r.stdout.split()[0].decode()


def main():
    spec = []
    for msg, want in SPEC:
        got = M.ripemd160(msg).hex()
        assert want is None or got == want, (msg[:20], got, want)
        assert openssl(msg) == got, (msg[:20], got)
        if len(msg) == 1000000:
            spec.append({"repeat": "a", "count": 1000000, "ripemd160": got})
        else:
            spec.append({"msg": msg.decode(), "ripemd160": got})
    rng = random.Random(160)
    rand = []
    for n in LENS:
        msg = bytes(rng.getrandbits(8) for _ in range(n))
        got = M.ripemd160(msg).hex()
        assert openssl(msg) == got, n
        rand.append({"len": n, "msg": msg.hex(), "ripemd160": got})
    msg = M.long_message(100000)
    got = M.ripemd160(msg).hex()
    assert openssl(msg) == got
    rand.append({"len": 100000, "long_message": 100000, "ripemd160": got})
    path = os.path.join(ROOT, "tests", "golden", "md_hashes.json")
    with open(path, "w") as f:
        json.dump({"spec": spec, "random": rand}, f, indent=0)
        f.write("\n")
    print(f"wrote {path}: {len(spec)} spec vectors, {len(rand)} seeded messages, all equal to openssl's")


if __name__ == "__main__":
    main()
