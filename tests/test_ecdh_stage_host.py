"""CPU check of the staging plans of gsv_secp256k1_scalar_mul_batch / gsv_ecdh_batch (csrc/staging.h
ScalarMulStage, EcdhStage): tests/native/ecdh_stage_host.cpp rebuilds both plans with the structs the
entry points use, for n in {1, 255, 256, 257, 2^20} and with and without each optional output, and checks
alignment, disjointness, sizes and the total, that the secret regions (scalars, then secret outputs) are
first and contiguous, and that the wipe length `secret` ends exactly at the last of them: what the host
forms' wipe of [0, secret) rests on.  A stand-alone program (g++, with ASan + UBSan when the compiler
links them), run as a child process."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "ecdh_stage_host.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def test_ecdh_stage_plans(tmp_path):
    exe = tmp_path / "ecdh_stage_host"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe), SRC]
    if subprocess.run(base + SAN, capture_output=True).returncode != 0:  # no sanitizer runtime: plain build
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok 20"), r.stdout  # 5 sizes x (1 scalar_mul plan + 3 ecdh plans)
