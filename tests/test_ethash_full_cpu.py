"""CPU tests of the sealing half of the ethash family: the sizing of the sealer's rounds (csrc/ethash_host.h) as a
stand-alone program, the new ABI values, and the argument checks that need no device."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_seal_rounds_as_a_program_under_sanitizers(tmp_path):
    """tests/native/ethash_seal_main.cpp with ASan + UBSan (a plain build where the compiler links neither),
    run as a child process"""
    src = os.path.join(ROOT, "tests", "native", "ethash_seal_main.cpp")
    exe = tmp_path / "ethash_seal_main"
    base = ["g++", "-O2", "-g", "-std=c++17", "-Wall", "-o", str(exe), src]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_abi_pins_of_the_sealing_half():
    from gsv import _lib
    txt = open(os.path.join(ROOT, "include", "gsv.h")).read()

    def val(name):
        return int(re.search(r"#define %s (\d+)" % name, txt).group(1))
    assert val("GSV_ST_NONCE_NOT_FOUND") == _lib.ST_NONCE_NOT_FOUND == 19
    assert _lib.ST_NONCE_NOT_FOUND in _lib.STATUS_STRINGS
    assert val("GSV_K_TOP") == _lib.K_TOP == 20  # pinned: the new ids are behind it
    assert val("GSV_K_ETHASH_FULL") == _lib.K_ETHASH_FULL == 20
    assert val("GSV_K_ETHASH_SEARCH") == _lib.K_ETHASH_SEARCH == 21
    assert val("GSV_K_ETHASH_FINISH") == _lib.K_ETHASH_FINISH == 22
    assert val("GSV_K_PEAK") == _lib.K_PEAK == 23
    assert val("GSV_ETHASH_MAX_DATASETS") == _lib.ETHASH_MAX_DATASETS == 2
    assert val("GSV_ETHASH_MAX_CACHES") == _lib.ETHASH_MAX_CACHES == 3


def test_entry_points_check_their_arguments():
    from gsv import _lib
    L = _lib.load()
    assert L.gsv_ctx_ethash_datasets(None, None) == _lib.E_INVALID_ARG
    assert L.gsv_ethash_full_batch(None, None, 0, None, None, 1, None, None) == _lib.E_INVALID_ARG
    assert L.gsv_ethash_seal_batch(None, None, 0, None, None, None, 1, 1, None, None, None) == _lib.E_INVALID_ARG
    assert L.gsv_ethash_full_batch_dev(None, None, 128, None, None, 1, None, None, None) == _lib.E_INVALID_ARG
    assert L.gsv_ethash_verify_seal_full_batch_dev(None, None, 128, None, None, None, None, 1, None,
                                                   None) == _lib.E_INVALID_ARG
    assert L.gsv_ethash_search_dev(None, None, 128, None, None, None, 1, 1, None, None, None, None, None,
                                   None) == _lib.E_INVALID_ARG
