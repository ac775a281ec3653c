"""CPU-only: the Philox stream arithmetic (flashe_amd/csrc/philox_stream.h: the counter and word of draw i, the state after n draws, the
blocks and tiles of a launch's segments, the 256-bit counter's carries and its wrap at 2^256) against a generator that walks the stream
one draw at a time, and the checks of a segment table (buffer_pos, segment count, overflowing counts, overlapping ranges), built with
AddressSanitizer + UBSan as a stand-alone program (tests/host_philox_stream_check.cpp)."""
import os
import subprocess

from conftest import ROOT


def test_philox_stream_against_a_one_by_one_walk_under_sanitizers(tmp_path):
    exe = tmp_path / "philox_stream_check"
    src = os.path.join(ROOT, "tests", "host_philox_stream_check.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "flashe_amd", "csrc"), src, "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "PHILOX_STREAM_OK 1640 draws" in r.stdout, r.stdout + r.stderr[-3000:]
