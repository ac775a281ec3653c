"""CPU test: the summed chain kernel that also writes the arbiter's decrypt mask (prf_chain_dmask_kernel, kernels.hip) keeps the
budget of the hot kernels -- no scratch, at most 128 VGPRs (four 1,024-thread waves per SIMD), the LDS of prf_chain_kernel -- per the
code objects inside the built library (tools/kernel_resources.py), and the headline summed kernel it sits beside is still there."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_dmask_kernel_budget():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.resources(os.path.join(ROOT, "flashe_amd", "libflashe_hip.so"))
    dm = [r for k, r in res.items() if "prf_chain_dmask_kernel<1024>" in k]
    assert len(dm) == 1, [k for k in res if "dmask" in k]
    r = dm[0]
    assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, r
    assert r["vgpr"] + r["agpr"] <= 128, r
    assert r["max_workgroup"] == 1024, r
    chain_sum = [r for k, r in res.items() if "prf_chain_kernel<1024, true, false>" in k]
    assert len(chain_sum) == 1 and r["lds_bytes_static"] == chain_sum[0]["lds_bytes_static"] == 133632, (r, chain_sum)
