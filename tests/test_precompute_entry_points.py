"""CPU: the entry points of the fused precompute client step are declared in include/flashe.h, exported by the built library and listed
in include/ENTRY_POINTS.md, and their kernels in the code objects keep to the streaming budget (no scratch, at most 128 VGPRs)."""
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "flashe_amd", "libflashe_hip.so")
ENTRY_POINTS = ["flashe_quantize_encrypt_prepared_model_dev", "flashe_quantize_encrypt_prepared_tensors_dev",
                "flashe_quantize_batch_encrypt_prepared_model_dev", "flashe_quantize_batch_encrypt_prepared_tensors_dev",
                "flashe_decrypt_prepared_unquantize_model_dev", "flashe_decrypt_prepared_unbatch_unquantize_model_dev"]
KERNELS = ["quantize_combine_model_kernel<", "combine_unquantize_model_kernel<", "quantize_batch_combine_model_kernel<",
           "combine_unbatch_unquantize_model_kernel<"]


def test_prepared_step_entry_points_are_declared_exported_and_indexed():
    from flashe_amd import _lib
    header = open(os.path.join(ROOT, "include", "flashe.h")).read()
    index = open(os.path.join(ROOT, "include", "ENTRY_POINTS.md")).read()
    nm = shutil.which("nm")
    exported = subprocess.run([nm, "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout.split() if nm else None
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header, name
        assert f"| `{name}` |" in index, name
        assert name in _lib.EXPORTED_SYMBOLS, name
        if exported is not None:
            assert name in exported, name
    if exported is None:
        import ctypes
        lib = ctypes.CDLL(LIB)
        assert all(hasattr(lib, name) for name in ENTRY_POINTS)


def test_prepared_step_kernels_keep_the_streaming_budget():
    if not (os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objcopy") and shutil.which("c++filt")):
        pytest.skip("llvm-readelf / llvm-objcopy / c++filt not found")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.resources(LIB)
    found = {k: r for k, r in res.items() if any(t in k for t in KERNELS)}
    assert len(found) == 2 * len(KERNELS), sorted(found)                      # the 128-bit and the one-limb instantiation of each
    for k, r in found.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, (k, r)
        assert r["vgpr"] + r["agpr"] <= 128, (k, r)
