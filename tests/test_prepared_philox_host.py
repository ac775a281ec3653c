"""CPU-only: the per-client draw plans of the prepared cohort launch that generates its own Philox draws (flashe_amd/csrc/philox_stream.h:
client_plan, client_draw, client_draws4, cohort_plans) and its staging block (layer_tables.h: prepared_block with plans) against a generator
that walks the stream one draw at a time -- every buffer_pos, client offsets of every residue, the counter's carry and its wrap -- and
the tiling check of the segments (gap, overlap, overrun), built with AddressSanitizer + UBSan as a stand-alone program
(tests/host_prepared_philox_check.cpp)."""
import os
import subprocess

from conftest import ROOT


def test_client_plans_and_the_staging_block_against_a_one_by_one_walk_under_sanitizers(tmp_path):
    exe = tmp_path / "prepared_philox_check"
    src = os.path.join(ROOT, "tests", "host_prepared_philox_check.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "flashe_amd", "csrc"), src, "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "PREPARED_PHILOX_OK" in r.stdout, r.stdout + r.stderr[-3000:]
