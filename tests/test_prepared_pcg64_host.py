"""CPU-only: the host arithmetic of the prepared cohort launch that generates its own PCG64 / PCG64DXSM draws
(flashe_amd/csrc/pcg64_stream.h: client_plan, cohort_plans, the lane walk -- workgroup_jump, lane_jump, stride_jump, next_pass, run_words).
First as a stand-alone program built with AddressSanitizer + UBSan (tests/host_prepared_pcg64_check.cpp) against a generator stepped one
draw at a time; then through the library's host entry point flashe_pcg64_cohort_lane_draws, which runs exactly the functions the kernel
compiles, against NumPy's own Generator.random for grids and lengths no test launches: both variants, lanes of the first, a middle and the
last workgroup, stretches that start at a draw that is no multiple of four.  Touches no device."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from flashe_amd.engine import Engine, FlasheError

M128 = 2 ** 128 - 1


def test_plans_and_the_lane_walk_against_a_one_by_one_walk_under_sanitizers(tmp_path):
    exe = tmp_path / "prepared_pcg64_check"
    src = os.path.join(ROOT, "tests", "host_prepared_pcg64_check.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "flashe_amd", "csrc"), src, "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "PREPARED_PCG64_OK" in r.stdout, r.stdout + r.stderr[-3000:]


def _gen(name, seed, pre=0, hand=None):
    g = np.random.Generator(getattr(np.random, name)(seed))
    if hand is not None:
        st = g.bit_generator.state
        st["state"]["state"], st["state"]["inc"] = hand
        g.bit_generator.state = st
    if pre:
        g.random(pre)
    return g


def _want(g, first, workgroups, run, iterations):
    """the draws of values 4 (run + 256 workgroups p) + i, p < iterations, of a client whose stretch starts `first` draws into g: NumPy's"""
    h = np.random.Generator(type(g.bit_generator)())
    h.bit_generator.state = g.bit_generator.state
    stream = h.random(first + 4 * (run + 256 * workgroups * (iterations - 1)) + 4)[first:]
    return np.concatenate([stream[4 * (run + 256 * workgroups * p):][:4] for p in range(iterations)])


@pytest.mark.parametrize("name", ["PCG64", "PCG64DXSM"])
@pytest.mark.parametrize("workgroups", [1, 3, 2048])
def test_the_lane_walk_is_numpys_stream(name, workgroups):
    """Three passes (two compositions with the stride jump) of lanes in the first, a middle and the last workgroup; the client's stretch
    starts 0, 1, 2, 3 and 1001 x 7 + 2 draws into a generator that has itself drawn already."""
    g = _gen(name, 11, pre=3)
    before = repr(g.bit_generator.state)
    runs = 256 * workgroups
    for first in (0, 1, 2, 3, 7009):
        for run in sorted({0, 1, 255, runs // 2 + 7 if workgroups > 1 else 77, runs - 256, runs - 1}):
            got = Engine.pcg64_cohort_lane_draws(g, first, workgroups, run, 3)
            assert got.dtype == np.float64 and np.array_equal(got, _want(g, first, workgroups, run, 3)), (first, run)
    assert repr(g.bit_generator.state) == before                                     # nothing is advanced


@pytest.mark.parametrize("name", ["PCG64", "PCG64DXSM"])
def test_states_set_by_hand_and_a_far_lane(name):
    """an even inc, inc 0, a state of 2^128 - 1; a state dict in place of a Generator; run 123,457 of 1,000 workgroups"""
    for hand in ((M128, 2 ** 64), (12345, 0), (0, M128), (0x0123456789ABCDEFFEDCBA9876543210, 2)):
        g = _gen(name, 5, hand=hand)
        for first in (0, 5):
            assert np.array_equal(Engine.pcg64_cohort_lane_draws(g, first, 3, 301, 4), _want(g, first, 3, 301, 4)), (hand, first)
            assert np.array_equal(Engine.pcg64_cohort_lane_draws(g.bit_generator.state, first, 1, 9, 2), _want(g, first, 1, 9, 2)), (hand, first)
    g = _gen(name, 6, pre=1)
    assert np.array_equal(Engine.pcg64_cohort_lane_draws(g, 2, 1000, 123457, 2), _want(g, 2, 1000, 123457, 2))
    assert Engine.pcg64_cohort_lane_draws(g, 2, 1000, 123457, 0).size == 0


def test_the_helper_refuses_what_no_launch_has():
    g = _gen("PCG64", 1)
    for first, workgroups, run in ((0, 0, 0), (0, 1, 256), (0, 3, 768), (2 ** 60 + 1, 1, 0)):
        with pytest.raises(FlasheError) as ei:
            Engine.pcg64_cohort_lane_draws(g, first, workgroups, run, 1)
        assert ei.value.code == -22
    with pytest.raises(FlasheError):
        Engine.pcg64_cohort_lane_draws(np.random.Generator(np.random.Philox(1)), 0, 1, 0, 1)
