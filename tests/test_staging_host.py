"""CPU check of the staging plans of the 14 host-pointer entry points (csrc/staging.h: one declaration
per staged device buffer, the total to reserve derived from those declarations): tests/native/
staging_host.cpp rebuilds each plan with the structs the entry points use, for n in {1, 3}, with every
optional output absent and present, the partition path with an empty local block, and the merge stage at
the end of gsv_ethash_verify_headers_batch (a status byte per header in each buffer), and checks that
every offset is 256-aligned, the buffers are pairwise disjoint, the last ends at or before the total,
and the temporary shape's offset is that total.  A stand-alone program (g++, with ASan + UBSan when
the compiler links them), run as a child process."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "staging_host.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def test_staging_plans(tmp_path):
    exe = tmp_path / "staging_host"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe), SRC]
    if subprocess.run(base + SAN, capture_output=True).returncode != 0:  # no sanitizer runtime: plain build
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
