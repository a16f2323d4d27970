"""CPU check of the staging plans of gsv_ecies_decrypt_batch / gsv_ecies_encrypt_batch (csrc/staging.h
EciesDecryptStage, EciesEncryptStage): tests/native/ecies_stage_host.cpp rebuilds both plans with the
structs the entry points use, for n in {1, 255, 256, 257, 2^20}, four item sizes (0 included) and with
and without an s2 table, and checks alignment, disjointness, sizes and the total, that the secret regions
(the keys, the work area that holds Ke || Km, the plaintext) are first and contiguous from offset 0, and
that the wipe length `secret` ends exactly at the last of them: what the host forms' wipe of [0, secret)
rests on.  A stand-alone program (g++, with ASan + UBSan when the compiler links them), run as a child
process."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "ecies_stage_host.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def test_ecies_stage_plans(tmp_path):
    exe = tmp_path / "ecies_stage_host"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe), SRC]
    if subprocess.run(base + SAN, capture_output=True).returncode != 0:  # no sanitizer runtime: plain build
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok 120"), r.stdout  # 5 sizes x 4 item sizes x 3 s2 modes x 2 plans
