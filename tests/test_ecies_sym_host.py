"""CPU check of the message half's device headers compiled for the host (csrc/ecies_sym_dev.cuh over
csrc/aes128_dev.cuh and csrc/sha256_dev.cuh): tests/native/ecies_sym_host.cpp, a stand-alone program
(g++, with ASan + UBSan when the compiler links them) run as a child process.  It is fed (Ke, Km, em, s2)
of every row of tests/golden/ecies.json that has them, and of the six RLPx packets, with em and s2 at
every pair of byte offsets 0 - 3 inside heap blocks that end with the strings' last dwords, in both
directions, and must print the fixture's tag and the message (or the ciphertext)."""
import os
import subprocess

import ecies_model as M
from conftest import ROOT, golden

SRC = os.path.join(ROOT, "tests", "native", "ecies_sym_host.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def _cases():
    """[(ke, km, em, s2, tag, msg)] as bytes"""
    fx = golden("ecies.json")
    out = []
    for r in fx["good"] + fx["bad"]:
        if "ke" not in r:
            continue
        ct = bytes.fromhex(r["ct"])
        out.append((bytes.fromhex(r["ke"]), bytes.fromhex(r["km"]), ct[65:-32], bytes.fromhex(r["s2"]),
                    bytes.fromhex(r["sym_tag"]), bytes.fromhex(r["sym_msg"])))
    rl = golden("ecies_rlpx.json")
    for p in rl["packets"]:
        raw = bytes.fromhex(p["packet"])
        s2, c = (raw[:2], raw[2:]) if p["eip8"] else (b"", raw)
        ke, km = M.keys_of(c[1:65], bytes.fromhex(rl[p["key"]]))
        out.append((ke, km, c[65:-32], s2, c[-32:], M.aes128_ctr(ke, c[65:81], c[81:-32])))
    return out


def _hex(b):
    return b.hex() if b else "-"


def test_sym_host_build_against_the_fixture(tmp_path):
    exe = tmp_path / "ecies_sym_host"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", str(exe), SRC]
    if subprocess.run(base + SAN, capture_output=True).returncode != 0:  # no sanitizer runtime: plain build
        subprocess.run(base, check=True)
    cases = _cases()
    assert len(cases) >= 45
    assert {len(c[5]) for c in cases} >= set(M.MSG_LENS)  # length 0: the len-113 rows
    lines, want = [], []
    for ke, km, em, s2, tag, msg in cases:
        iv, body = em[:16], em[16:]
        for od, os_ in [(a, b) for a in range(4) for b in range(4)]:  # every pair of offsets, every case
            lines.append(f"d {ke.hex()} {km.hex()} {iv.hex()} {_hex(body)} {_hex(s2)} {od} {os_}")
            want.append(f"{tag.hex()} {_hex(msg)}")
            lines.append(f"e {ke.hex()} {km.hex()} {iv.hex()} {_hex(msg)} {_hex(s2)} {od} {os_}")
            want.append(f"{tag.hex()} {_hex(body)}")
    r = subprocess.run([str(exe)], input="".join(x + "\n" for x in lines), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    for ln, w, g in zip(lines, want, got):
        assert g == w, ln[:120]
    # a malformed line is refused, not read past
    r = subprocess.run([str(exe)], input="d abcd\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
