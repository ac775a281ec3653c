"""CPU test: the kernels of the prepared cohort's online launch that generates its own PCG64 / PCG64DXSM draws
(quantize_pcg64_combine_cohort_kernel, codec.hip) are streaming kernels -- once per element type and variant, no scratch, no spills, no LDS,
at most 128 VGPRs -- per the code objects inside the built library (tools/kernel_resources.py); the entry points are in the header, the
library, the binding and the index.  No exact register count is pinned."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "quantize_pcg64_combine_cohort_kernel<"
ENTRY_POINTS = ["flashe_quantize_combine_cohort_pcg64_dev", "flashe_quantize_combine_cohort_pcg64_u32_dev", "flashe_pcg64_cohort_grid",
                "flashe_pcg64_cohort_lane_draws"]
OTHERS = ["quantize_combine_cohort_kernel<", "quantize_batch_combine_cohort_kernel<", "quantize_philox_combine_cohort_kernel<",
          "quantize_batch_philox_combine_cohort_kernel<"]


def test_inline_draw_kernels_keep_the_streaming_budget():
    if not (os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objcopy") and shutil.which("c++filt")):
        pytest.skip("llvm-readelf / llvm-objcopy / c++filt not found")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.resources(os.path.join(ROOT, "flashe_amd", "libflashe_hip.so"))
    found = {k: r for k, r in res.items() if KERNEL in k}
    # once per element type -- uint32 (compact), uint64 (one limb), unsigned __int128 (two limbs) -- and variant
    assert len(found) == 6, sorted(found)
    for elem in ("<unsigned int,", "<unsigned long,", "<unsigned __int128,"):
        for variant in ("Variant)0>", "Variant)1>"):
            assert sum(elem in k and variant in k for k in found) == 1, (elem, variant, sorted(found))
    # the names the buffer and Philox forms' tests count by do not match the new kernels
    assert not any(other in k for other in OTHERS for k in found)
    for k, r in found.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, (k, r)
        assert r["lds_bytes_static"] == 0, (k, r)
        assert r["vgpr"] + r["agpr"] <= 128, (k, r)


def test_the_entry_points_are_declared_bound_indexed_and_exported():
    header = open(os.path.join(ROOT, "include", "flashe.h")).read()
    index = open(os.path.join(ROOT, "include", "ENTRY_POINTS.md")).read()
    from flashe_amd import _lib
    from flashe_amd.engine import Engine
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header
        assert f"| `{name}` |" in index
        assert name in _lib._SIGNATURES
    for method in ("quantize_combine_cohort_pcg64_dev", "pcg64_cohort_grid", "pcg64_cohort_lane_draws"):
        assert hasattr(Engine, method)
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert all(hasattr(lib, name) for name in ENTRY_POINTS)
