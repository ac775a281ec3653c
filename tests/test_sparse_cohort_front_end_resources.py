"""CPU test: prf_small_sparse_cohort_kernel<B>, the sparse cohort's chained quantise + encrypt launch, is compiled at the five widths of the
compact chain and keeps the small chain's budget -- 1,024-thread workgroups, no scratch, no VGPR spills, at most 128 VGPRs -- per the code
objects inside the built library (tools/kernel_resources.py); and the entry point that launches it is exported, bound and indexed without
an ABI bump."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "flashe_amd", "libflashe_hip.so")
SYM = "flashe_quantize_encrypt_sparse_cohort_dev"
WIDTHS = (16, 20, 23, 24, 32)


def test_sparse_cohort_front_end_kernel_budget():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("the ROCm LLVM tools are not installed")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.resources(LIB)
    hits = {k: r for k, r in res.items() if "flashe::prf_small_sparse_cohort_kernel<" in k}
    assert sorted(int(re.search(r"prf_small_sparse_cohort_kernel<(\d+)>", k).group(1)) for k in hits) == sorted(WIDTHS), sorted(hits)
    for k, r in hits.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, (k, r)
        assert r["vgpr"] + r["agpr"] <= 128, (k, r)
        assert r["max_workgroup"] == 1024, (k, r)
    # the name hides from the counts of the kernels next to it (test_cohort_compact_resources.py, test_sparse_cohort_resources.py)
    assert not [k for k in hits if "prf_small_cohort_kernel<" in k or "quantize_cohort_kernel" in k]
    # the LDS is the small chain's
    chain = [r for k, r in res.items() if "flashe::prf_small_cohort_kernel<" in k]
    assert chain and {r["lds_bytes_static"] for r in hits.values()} == {r["lds_bytes_static"] for r in chain}


def test_entry_point_is_exported_bound_and_indexed():
    from flashe_amd import _lib
    assert SYM in _lib.EXPORTED_SYMBOLS and SYM in _lib._SIGNATURES
    assert hasattr(_lib.load(), SYM)
    index = open(os.path.join(ROOT, "include", "ENTRY_POINTS.md")).read()
    header = open(os.path.join(ROOT, "include", "flashe.h")).read()
    assert SYM in index and SYM in header
    dyn = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert f" T {SYM}" in dyn
    assert _lib.load().flashe_abi_version() == 4
