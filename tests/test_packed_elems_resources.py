"""CPU: the two entry points of the packed reduce on unpacked vectors are declared in include/flashe.h, exported by the built library,
bound in flashe_amd/_lib.py and listed in include/ENTRY_POINTS.md with the reference lines their comment cites; the ABI version is still
4; and their kernels in the code object keep to the streaming budget (no scratch, at most 128 VGPRs) in all three layouts."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "flashe_amd", "libflashe_hip.so")
ENTRY_POINTS = ["flashe_aggregate_packed_elems_dev", "flashe_aggregate_packed_elems_u32_dev"]
# stage 1 in the compact (four elements per lane, and one), one-limb and two-limb layouts (the last with 16-byte and with 8-byte operand loads), stage 2 in each layout
KERNELS = ["aggregate_packed_elems_u32x4_kernel(", "aggregate_packed_elems_kernel<0, false>(", "aggregate_packed_elems_kernel<1, false>(", "aggregate_packed_elems_kernel<2, true>(",
           "aggregate_packed_elems_kernel<2, false>(", "packed_elems_fixup_kernel<0>(", "packed_elems_fixup_kernel<1>(", "packed_elems_fixup_kernel<2>("]


def test_packed_elems_entry_points_are_declared_exported_bound_and_indexed():
    import ctypes
    from flashe_amd import _lib
    header = open(os.path.join(ROOT, "include", "flashe.h")).read()
    index = open(os.path.join(ROOT, "include", "ENTRY_POINTS.md")).read()
    nm = shutil.which("nm")
    exported = subprocess.run([nm, "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout.split() if nm else None
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header, name
        assert f"| `{name}` | jzf_aggregator.py:406-419" in index, name
        assert name in _lib.EXPORTED_SYMBOLS and name in _lib._SIGNATURES, name
        if exported is not None:
            assert name in exported, name
    if exported is not None:
        # the library exports exactly the header's names
        declared = set(re.findall(r"^(?:int|const char \*|void|uint64_t|size_t|unsigned)\s*\*?\s*(flashe_\w+)\s*\(", header, re.M))
        assert {s for s in exported if s.startswith("flashe_")} == declared
    lib = ctypes.CDLL(LIB)
    assert all(hasattr(lib, name) for name in ENTRY_POINTS)
    assert "#define FLASHE_ABI_VERSION 4\n" in header and lib.flashe_abi_version() == 4
    from flashe_amd.engine import Engine
    assert all(hasattr(Engine, name[len("flashe_"):]) for name in ENTRY_POINTS)


def test_packed_elems_kernels_keep_the_streaming_budget():
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
        # no LDS beyond the exchange arrays: one uint32 per lane and two words per wave
        assert r["lds_bytes_static"] <= 4 * 256 + 2 * 4 * 4, (k, r)
