"""CPU test: the PCG64 / PCG64DXSM draw launch (pcg64.hip).  Its entry points are bound in flashe_amd/_lib.py and listed in
include/ENTRY_POINTS.md, and its four kernels (pcg64_random_args_kernel, the plan table in the kernel arguments, and
pcg64_random_table_kernel, the table in device memory, for either variant) use no scratch, spill no VGPR, hold no static LDS and stay
inside the streaming kernels' 128 VGPRs, per the code objects inside the built library (tools/kernel_resources.py).  A dynamically indexed
by-value table that the compiler copied to the stack, or a 128-bit product it could not keep in registers, would show up here."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["flashe_pcg64_random_dev", "flashe_pcg64_advance", "flashe_pcg64_grid"]
KERNELS = ["pcg64_random_args_kernel", "pcg64_random_table_kernel"]


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_the_entry_points_are_bound_listed_and_declared(name):
    from flashe_amd import _lib
    assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.load(), name)
    with open(os.path.join(ROOT, "include", "ENTRY_POINTS.md")) as f:
        rows = [l for l in f if l.startswith(f"| `{name}` |")]
    assert len(rows) == 1 and rows[0].split("|")[2].strip() == "new", rows
    with open(os.path.join(ROOT, "include", "flashe.h")) as f:
        assert re.search(r"^int " + name + r"\(", f.read(), re.M)


@pytest.fixture(scope="module")
def resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    return kernel_resources.resources(os.path.join(ROOT, "flashe_amd", "libflashe_hip.so"))


@pytest.mark.parametrize("variant", [0, 1], ids=["pcg64", "dxsm"])
@pytest.mark.parametrize("name", KERNELS)
def test_the_pcg64_kernels_are_registers_only(resources, name, variant):
    hit = [r for r in resources.values() if f"{name}ILN12flashe_pcg647VariantE{variant}EE" in r["mangled"]]
    assert len(hit) == 1, (name, variant, [k for k in resources if "pcg64" in k])
    r = hit[0]
    assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, r
    assert r["lds_bytes_static"] == 0, r
    assert r["vgpr"] + r["agpr"] <= 128, r                    # the streaming kernels' budget
    assert r["max_workgroup"] == 256, r
