"""CPU-only: the table arithmetic the prepared cohort launches added to flashe_amd/csrc/layer_tables.h (prepared_block: where the mask
pointers, the ciphertext pointers and the batched rows lie in the block uploaded behind the cohort's tables; cohort_sources), built with
AddressSanitizer + UBSan (tests/host_prepared_block_check.cpp)."""
import os
import subprocess

from conftest import ROOT


def test_prepared_block_layout_under_sanitizers(tmp_path):
    exe = tmp_path / "prepared_block_check"
    src = os.path.join(ROOT, "tests", "host_prepared_block_check.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "flashe_amd", "csrc"), src, "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "PREPARED_BLOCK_OK" in r.stdout, r.stdout + r.stderr[-3000:]
