"""CPU test: the two instantiations of the Philox draw launch (philox.hip: philox_random_args_kernel, its plan table in the kernel
arguments, and philox_random_table_kernel, the table in device memory) use no scratch, spill no VGPR and hold no static LDS -- the kernel
is registers, multiplies and stores -- per the code objects inside the built library (tools/kernel_resources.py).  A dynamically indexed
by-value table that the compiler copied to the stack would show up here as scratch."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["philox_random_args_kernel", "philox_random_table_kernel"]


@pytest.fixture(scope="module")
def resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    return kernel_resources.resources(os.path.join(ROOT, "flashe_amd", "libflashe_hip.so"))


@pytest.mark.parametrize("name", KERNELS)
def test_the_philox_kernels_are_registers_only(resources, name):
    hit = [r for k, r in resources.items() if name + "(" in k]
    assert len(hit) == 1, (name, [k for k in resources if "philox" in k])
    r = hit[0]
    assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, r
    assert r["lds_bytes_static"] == 0, r
    assert r["vgpr"] + r["agpr"] <= 64, r                     # eight waves per SIMD: the launch hides its multiply latency by occupancy
    assert r["max_workgroup"] == 256, r
