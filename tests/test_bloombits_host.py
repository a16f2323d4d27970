"""CPU check of csrc/bloombits_host.h, the one place the bloombits family's host arithmetic lives:
tests/native/bloombits_host_main.cpp drops rules the way NewMatcher does over every combination of empty, nil and
plain clauses in up to three rules, packs compressed slots behind an offset table (in place too), and checks the
table, bloom and match sizes at the bounds of the section size and past 32 bits.  A stand-alone program (g++, with
ASan + UBSan when the compiler links them), run as a child process."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "bloombits_host_main.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def test_bloombits_host_arithmetic(tmp_path):
    exe = tmp_path / "bloombits_host_main"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe), SRC]
    if subprocess.run(base + SAN, capture_output=True).returncode != 0:  # no sanitizer runtime: plain build
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
