"""CPU test: the sparsifier kernels over caller-owned layers (spt_*_kernel, sparsify.hip) keep the budget of the batch passes they
mirror -- no scratch, no VGPR spills, at most 128 VGPRs -- per the code objects inside the built library (tools/kernel_resources.py)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sparsify_tensors_kernel_budget():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("the ROCm LLVM tools are not installed")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.resources(os.path.join(ROOT, "flashe_amd", "libflashe_hip.so"))
    spt = {k: r for k, r in res.items() if "flashe::spt_" in k}
    for stage in ("spt_hist_kernel<float>", "spt_hist_kernel<double>", "spt_count_kernel<float>", "spt_count_kernel<double>",
                  "spt_write_kernel<float>", "spt_write_kernel<double>", "spt_pick_digit_kernel", "spt_pack_kernel"):
        assert len([k for k in spt if stage in k]) == 1, (stage, sorted(spt))
    for k, r in spt.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, (k, r)
        assert r["vgpr"] + r["agpr"] <= 128, (k, r)
