"""CPU-only: the stream table of a cohort round with dropped-out clients (flashe_amd/csrc/cohort_streams.h: the streams a strictly
ascending index list needs, which of them complete an output, which open a run, the link each finishes and the number of runs) against a
brute-force closed form for every non-empty subset of ten clients at first_idx 0 and 2^32 - 12, and its refusals (unsorted, duplicate,
index 2^32 - 1, one run too many), built with AddressSanitizer + UBSan (tests/host_cohort_streams_check.cpp)."""
import os
import subprocess

from conftest import ROOT


def test_cohort_streams_against_closed_forms_under_sanitizers(tmp_path):
    exe = tmp_path / "cohort_streams_check"
    src = os.path.join(ROOT, "tests", "host_cohort_streams_check.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "flashe_amd", "csrc"), src, "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "COHORT_STREAMS_OK 2046 subsets" in r.stdout, r.stdout + r.stderr[-3000:]
