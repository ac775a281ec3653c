"""CPU test: the kernels of the BATCHED prepared cohort's online launch that generates its own Philox draws
(quantize_batch_philox_combine_cohort_kernel, codec.hip) are streaming kernels -- once per (element type, values per element), no
scratch, no spills, no LDS, at most 128 VGPRs -- per the code objects inside the built library (tools/kernel_resources.py); the entry
point is in the header, the library, the binding and the index.  No exact register count is pinned."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "quantize_batch_philox_combine_cohort_kernel<"
ENTRY_POINT = "flashe_quantize_batch_combine_cohort_philox_dev"


def test_batched_inline_draw_kernels_keep_the_streaming_budget():
    if not (os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objcopy") and shutil.which("c++filt")):
        pytest.skip("llvm-readelf / llvm-objcopy / c++filt not found")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.resources(os.path.join(ROOT, "flashe_amd", "libflashe_hip.so"))
    found = {k: r for k, r in res.items() if KERNEL in k}
    # once per element type -- uint64 (one limb), unsigned __int128 (two limbs); there is no compact batched layout -- and BS 5, 6, 7, 0
    assert len(found) == 8, sorted(found)
    for elem in ("<unsigned long,", "<unsigned __int128,"):
        for bs in (5, 6, 7, 0):
            assert sum(f"{elem} {bs}>" in k for k in found) == 1, (elem, bs, sorted(found))
    # the names the sibling kernels' tests count by do not match the new kernels
    for other in ("quantize_philox_combine_cohort_kernel<", "quantize_batch_combine_cohort_kernel<", "quantize_combine_cohort_kernel<"):
        assert not any(other in k for k in found)
        assert sum(other in k for k in res) == {"quantize_philox_combine_cohort_kernel<": 3, "quantize_batch_combine_cohort_kernel<": 8,
                                                "quantize_combine_cohort_kernel<": 3}[other]
    for k, r in found.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, (k, r)
        assert r["lds_bytes_static"] == 0, (k, r)
        assert r["vgpr"] + r["agpr"] <= 128, (k, r)


def test_the_entry_point_is_declared_bound_indexed_and_exported():
    header = open(os.path.join(ROOT, "include", "flashe.h")).read()
    index = open(os.path.join(ROOT, "include", "ENTRY_POINTS.md")).read()
    from flashe_amd import _lib
    from flashe_amd.engine import Engine
    assert f"int {ENTRY_POINT}(" in header
    assert f"| `{ENTRY_POINT}` |" in index
    assert ENTRY_POINT in _lib._SIGNATURES
    assert hasattr(Engine, "quantize_batch_combine_cohort_philox_dev")
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.load(), ENTRY_POINT)
