"""CPU test: the kernels FlasheSparseCohort adds (quantize_cohort_kernel in tensors.hip, spc_pack_kernel in sparsify.hip) keep the budget
of the streaming passes next to them -- no scratch, no VGPR spills, at most 128 VGPRs -- per the code objects inside the built library
(tools/kernel_resources.py), and the two entry points that launch them are exported, bound and indexed."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "flashe_amd", "libflashe_hip.so")
NEW = ("flashe_sparsify_cohort_tensors_dev", "flashe_quantize_cohort_dev")


def test_sparse_cohort_kernel_budget():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("the ROCm LLVM tools are not installed")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.resources(LIB)
    for name in ("flashe::quantize_cohort_kernel", "flashe::spc_pack_kernel"):
        hits = {k: r for k, r in res.items() if name in k}
        assert len(hits) == 1, (name, sorted(hits))
        (k, r), = hits.items()
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, (k, r)
        assert r["vgpr"] + r["agpr"] <= 128, (k, r)
    # the new names hide no existing stage from the counts of test_sparse_tensors_resources.py
    assert not [k for k in res if "flashe::spt_" in k and ("spc_" in k or "quantize_cohort" in k)]


def test_entry_points_are_exported_bound_and_indexed():
    from flashe_amd import _lib
    for sym in NEW:
        assert sym in _lib.EXPORTED_SYMBOLS and sym in _lib._SIGNATURES
        assert hasattr(_lib.load(), sym)
    index = open(os.path.join(ROOT, "include", "ENTRY_POINTS.md")).read()
    header = open(os.path.join(ROOT, "include", "flashe.h")).read()
    for sym in NEW:
        assert sym in index and sym in header
    dyn = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    for sym in NEW:
        assert f" T {sym}" in dyn
    assert _lib.load().flashe_abi_version() == 4
