"""CPU test: the kernels of the prepared cohort's online launch (quantize_combine_cohort_kernel, quantize_batch_combine_cohort_kernel,
codec.hip) are streaming kernels -- no scratch, no spills, no LDS, at most 128 VGPRs -- per the code objects inside the built library
(tools/kernel_resources.py).  No exact count is pinned."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["quantize_combine_cohort_kernel<", "quantize_batch_combine_cohort_kernel<"]


def test_prepared_cohort_kernels_keep_the_streaming_budget():
    if not (os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objcopy") and shutil.which("c++filt")):
        pytest.skip("llvm-readelf / llvm-objcopy / c++filt not found")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.resources(os.path.join(ROOT, "flashe_amd", "libflashe_hip.so"))
    found = {k: r for k, r in res.items() if any(t in k for t in KERNELS)}
    # the three element types of the un-batched kernel; the one-limb and the two-limb batched kernel at the compiled sizes and the run-time one
    assert sum("quantize_combine_cohort_kernel<" in k for k in found) == 3, sorted(found)
    assert sum("quantize_batch_combine_cohort_kernel<" in k for k in found) == 8, sorted(found)
    for k, r in found.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, (k, r)
        assert r["lds_bytes_static"] == 0, (k, r)
        assert r["vgpr"] + r["agpr"] <= 128, (k, r)
