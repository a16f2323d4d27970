"""CPU check of the staging plans of gsv_ecdsa_sign_batch / gsv_pubkey_create_batch (csrc/staging.h
SignStage, PubkeyCreateStage): tests/native/sign_stage_host.cpp rebuilds both plans with the structs the
entry points use and checks alignment, disjointness, sizes and the total, and that the secret keys are
the first region, alone in their slots: what the host forms' wipe of [0, 32 n) rests on.  A stand-alone
program (g++, with ASan + UBSan when the compiler links them), run as a child process."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "sign_stage_host.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def test_sign_stage_plans(tmp_path):
    exe = tmp_path / "sign_stage_host"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe), SRC]
    if subprocess.run(base + SAN, capture_output=True).returncode != 0:  # no sanitizer runtime: plain build
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok 15"), r.stdout
