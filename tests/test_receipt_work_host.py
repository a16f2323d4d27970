"""CPU check of csrc/receipt_host.h, the one place the receipt path's slot and work-area arithmetic lives:
tests/native/receipt_work_main.cpp packs bloom items of 21 and 33 bytes at every start offset and several gaps into
a heap table of exactly slot_count entries (no two in one slot, none past the end, the position recoverable from
slot and remainder) and checks the work area's three arrays for overlap, alignment and the two bounds.  A
stand-alone program (g++, with ASan + UBSan when the compiler links them), run as a child process."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "receipt_work_main.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def test_receipt_work_area(tmp_path):
    exe = tmp_path / "receipt_work_main"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe), SRC]
    if subprocess.run(base + SAN, capture_output=True).returncode != 0:  # no sanitizer runtime: plain build
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
