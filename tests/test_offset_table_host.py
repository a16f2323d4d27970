"""CPU check of csrc/offset_table.h, the one place the host forms' rule for a caller's offset table lives:
tests/native/offset_table_main.cpp runs the table check under every entry point's rule (n in {1, 3}, a
nonzero first entry, a step backwards at the first, middle and last entry, null data behind an all-empty and a
non-empty table, an item of exactly each cap and one byte more, a 2^33-byte item in the uncapped mode) and
compares the code with the one those entry points return; the rebased copy; and the right-padded fixed
records for item lengths 0, rec - 1, rec, rec + 1 with a guard byte on either side of the output.  A
stand-alone program (g++, with ASan + UBSan when the compiler links them), run as a child process."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "offset_table_main.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def test_offset_table_rules(tmp_path):
    exe = tmp_path / "offset_table_main"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe), SRC]
    if subprocess.run(base + SAN, capture_output=True).returncode != 0:  # no sanitizer runtime: plain build
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
