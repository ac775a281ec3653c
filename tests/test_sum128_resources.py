"""CPU test: the int_bits = 128 specialisation of the summed decrypt-mask chain (prf_dmask_sum128_kernel, kernels.hip) keeps the budget
of the kernel it replaces at that shape -- no scratch, at most 128 VGPRs (four 1,024-thread waves per SIMD), the LDS of
prf_chain_dmask_kernel and prf_chain_kernel -- per the code objects inside the built library (tools/kernel_resources.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sum128_kernel_budget():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.resources(os.path.join(ROOT, "flashe_amd", "libflashe_hip.so"))
    sp = [r for k, r in res.items() if "prf_dmask_sum128_kernel<1024>" in k]
    assert len(sp) == 1, [k for k in res if "sum128" in k]
    r = sp[0]
    assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, r
    assert r["vgpr"] + r["agpr"] <= 128, r
    assert r["max_workgroup"] == 1024, r
    dm = [v for k, v in res.items() if "prf_chain_dmask_kernel<1024>" in k]
    assert len(dm) == 1 and r["lds_bytes_static"] == dm[0]["lds_bytes_static"] == 133632, (r, dm)
