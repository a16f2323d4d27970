"""CPU check of the ECIES key derivation's device header compiled for the host (csrc/ecies_kdf.cuh over
csrc/sha256_dev.cuh): tests/native/ecies_kdf_host.cpp, a stand-alone program (g++, with ASan + UBSan when
the compiler links them) run as a child process.  It is fed every successful row's shared secret of
tests/golden/secp_ecdh.json on stdin, plus an all-zero and an all-0xFF X, and must print the fixture's
keys48 (hashlib's) for each."""
import hashlib
import os
import subprocess

from conftest import ROOT, golden

SRC = os.path.join(ROOT, "tests", "native", "ecies_kdf_host.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def _keys48(x: bytes) -> bytes:
    k = hashlib.sha256(b"\x00\x00\x00\x01" + x).digest()
    return k[:16] + hashlib.sha256(k[16:]).digest()


def test_kdf_host_build_against_the_fixture(tmp_path):
    exe = tmp_path / "ecies_kdf_host"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", str(exe), SRC]
    if subprocess.run(base + SAN, capture_output=True).returncode != 0:  # no sanitizer runtime: plain build
        subprocess.run(base, check=True)
    rows = [r for r in golden("secp_ecdh.json")["rows"] if r["status"] == 0]
    assert len(rows) >= 80
    cases = [(r["shared"], r["keys48"]) for r in rows]
    for x in (bytes(32), b"\xff" * 32, bytes(31) + b"\x01"):
        cases.append((x.hex(), _keys48(x).hex()))
    r = subprocess.run([str(exe)], input="".join(x + "\n" for x, _ in cases), capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    got = r.stdout.split()
    assert len(got) == len(cases)
    for (x, want), g in zip(cases, got):
        assert g == want, x
    # a malformed line is refused, not read past
    r = subprocess.run([str(exe)], input="abcd\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
