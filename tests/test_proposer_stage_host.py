"""CPU check of the staging plans of gsv_proposer_create_collations, gsv_blob_serialize_batch and
gsv_blob_deserialize_batch (csrc/staging.h ProposerStage, BlobSerStage, BlobDeserStage):
tests/native/proposer_stage_host.cpp rebuilds the plans with the structs the entry points use and checks
alignment, disjointness, sizes and the total, and that the proposer's secret keys are the first region,
alone in their slots: what the host form's wipe of [0, 32 n) rests on.  A stand-alone program (g++, with
ASan + UBSan when the compiler links them), run as a child process."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "proposer_stage_host.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def test_proposer_stage_plans(tmp_path):
    exe = tmp_path / "proposer_stage_host"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe), SRC]
    if subprocess.run(base + SAN, capture_output=True).returncode != 0:  # no sanitizer runtime: plain build
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok 60"), r.stdout  # 5 sizes x (3 x (1 proposer + 2 serialize) + 3 deserialize)
