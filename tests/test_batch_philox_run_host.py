"""CPU-only: the run arithmetic of the batched prepared cohort launch that generates its own Philox draws (flashe_amd/csrc/philox_stream.h:
client_run, RunWalk, RunBlocks; layer_tables.h: batched_groups, prepared_block with groups and plans) against brute force -- position() + block(),
value by value -- at every skip, bs 1 .. 10 and 128, row starts 0 .. 7, runs that end in pads, the counter's carry and its wrap; and
cohort_plans' refusal of a table that tiles the elements instead of the values.  Built with AddressSanitizer + UBSan as a stand-alone
program (tests/host_batch_philox_run_check.cpp)."""
import os
import subprocess

from conftest import ROOT


def test_run_arithmetic_against_brute_force_under_sanitizers(tmp_path):
    exe = tmp_path / "batch_philox_run_check"
    src = os.path.join(ROOT, "tests", "host_batch_philox_run_check.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "flashe_amd", "csrc"), src, "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "BATCH_PHILOX_RUN_OK" in r.stdout, r.stdout + r.stderr[-3000:]
