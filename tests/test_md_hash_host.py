"""CPU check of the Merkle-Damgard device headers compiled for the host (csrc/md_block_dev.cuh,
csrc/ripemd160_dev.cuh, csrc/sha256_dev.cuh): tests/native/md_hash_host.cpp, a stand-alone program (g++, with
ASan + UBSan when the compiler links them) run as a child process.  It hashes messages of every length
0 - 200 and of 247, 248, 311 and 312 bytes (one and two padding blocks behind one to four message blocks)
at byte offsets 0 - 3, each in a heap block that ends with the message's last byte, and must print what
hashlib.sha256 and tests/ripemd160_model.py give."""
import hashlib
import os
import subprocess

import numpy as np

import ripemd160_model as M
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "md_hash_host.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
LENS = list(range(201)) + [247, 248, 311, 312]


def test_md_host_build_against_hashlib_and_the_model(tmp_path):
    exe = tmp_path / "md_hash_host"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", str(exe), SRC]
    if subprocess.run(base + SAN, capture_output=True).returncode != 0:  # no sanitizer runtime: plain build
        subprocess.run(base, check=True)
    rng = np.random.default_rng(256160)
    lines, want = [], []
    for n in LENS:
        msg = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        for shift in range(4):
            for kind, dig in (("s", hashlib.sha256(msg).hexdigest()), ("r", M.ripemd160(msg).hex())):
                lines.append(f"{kind} {msg.hex() or '-'} {shift}")
                want.append(dig)
    r = subprocess.run([str(exe)], input="".join(x + "\n" for x in lines), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    for ln, w, g in zip(lines, want, got):
        assert g == w, ln[:80]
    # a malformed line is refused, not read past
    for bad in ("s abc 0\n", "x 00 0\n", "r 00 4\n", "s 00\n"):
        r = subprocess.run([str(exe)], input=bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, bad
