"""CPU-only: the arithmetic of the per-layer tables behind the layered entry points (flashe_amd/csrc/layer_tables.h: layer ends, batched
element counts, the sparsifier's block layout, blob and stage-slot offsets) against closed forms, built with AddressSanitizer + UBSan
(tests/host_layer_tables_check.cpp)."""
import os
import subprocess

from conftest import ROOT


def test_layer_tables_against_closed_forms_under_sanitizers(tmp_path):
    exe = tmp_path / "layer_tables_check"
    src = os.path.join(ROOT, "tests", "host_layer_tables_check.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "flashe_amd", "csrc"), src, "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "LAYER_TABLES_OK" in r.stdout, r.stdout + r.stderr[-3000:]
