"""CPU-only: the PCG64 / PCG64DXSM stream arithmetic (flashe_amd/csrc/pcg64_stream.h: the step and the two output functions, the jump over
k steps by doubling, the state after n draws, the jump tables and the route the device launch takes to a draw, at states and increments of
0 and 2^128 - 1 and at even increments, jump(a + b) = jump(b) o jump(a) at distances up to 2^127) against a generator that walks the
stream one draw at a time, and the checks of a segment table (variant, segment count, overflowing counts, overlapping ranges), built with
AddressSanitizer + UBSan as a stand-alone program (tests/host_pcg64_stream_check.cpp)."""
import os
import subprocess

from conftest import ROOT


def test_pcg64_stream_against_a_one_by_one_walk_under_sanitizers(tmp_path):
    exe = tmp_path / "pcg64_stream_check"
    src = os.path.join(ROOT, "tests", "host_pcg64_stream_check.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "flashe_amd", "csrc"), src, "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "PCG64_STREAM_OK 235776 draws" in r.stdout, r.stdout + r.stderr[-3000:]
