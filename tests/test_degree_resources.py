"""CPU: the two entry points of the aggregator's degree scaling are declared in include/flashe.h, exported by the built library, bound in
flashe_amd/_lib.py and listed in include/ENTRY_POINTS.md, and their kernels in the code objects keep to the streaming budget (no scratch,
at most 128 VGPRs)."""
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "flashe_amd", "libflashe_hip.so")
ENTRY_POINTS = ["flashe_stage_layers_dev", "flashe_finish_layers_dev"]
KERNELS = ["stage_rows_kernel(", "finish_layers_kernel(", "finish_stat_blocks_kernel(", "finish_stat_combine_kernel("]


def test_degree_entry_points_are_declared_exported_bound_and_indexed():
    from flashe_amd import _lib
    header = open(os.path.join(ROOT, "include", "flashe.h")).read()
    index = open(os.path.join(ROOT, "include", "ENTRY_POINTS.md")).read()
    nm = shutil.which("nm")
    exported = subprocess.run([nm, "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout.split() if nm else None
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header, name
        assert f"| `{name}` | jzf_aggregator.py:" in index, name            # with the reference lines its comment cites
        assert name in _lib.EXPORTED_SYMBOLS and name in _lib._SIGNATURES, name
        if exported is not None:
            assert name in exported, name
    if exported is None:
        import ctypes
        lib = ctypes.CDLL(LIB)
        assert all(hasattr(lib, name) for name in ENTRY_POINTS)
    # the row structs of the binding have the header's layout: 48 and 64 bytes
    import ctypes
    assert ctypes.sizeof(_lib.StageRow) == 48 and ctypes.sizeof(_lib.FinishRow) == 64
    for flag, value in [("FLASHE_STAGE_SCALE", _lib.STAGE_SCALE), ("FLASHE_STAGE_SCALE_WIDE", _lib.STAGE_SCALE_WIDE), ("FLASHE_STAGE_SHIFT", _lib.STAGE_SHIFT),
                        ("FLASHE_STAGE_SHIFT_WIDE", _lib.STAGE_SHIFT_WIDE), ("FLASHE_STAGE_OUT_F64", _lib.STAGE_OUT_F64),
                        ("FLASHE_FINISH_DIV_TOTAL", _lib.FINISH_DIV_TOTAL), ("FLASHE_FINISH_SHIFT", _lib.FINISH_SHIFT),
                        ("FLASHE_FINISH_DIV_OWN", _lib.FINISH_DIV_OWN), ("FLASHE_FINISH_ADD_LAST", _lib.FINISH_ADD_LAST)]:
        assert f"#define {flag} {value}\n" in header, flag


def test_degree_kernels_keep_the_streaming_budget():
    if not (os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objcopy") and shutil.which("c++filt")):
        pytest.skip("llvm-readelf / llvm-objcopy / c++filt not found")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.resources(LIB)
    found = {k: r for k, r in res.items() if any(t in k for t in KERNELS)}
    assert len(found) == len(KERNELS), sorted(found)
    for k, r in found.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, (k, r)
        assert r["vgpr"] + r["agpr"] <= 128, (k, r)
