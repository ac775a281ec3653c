"""CPU test: prf_dec_sum128_kernel (kernels.hip) -- the headline summed chain that stores the decrypted sum where
prf_dmask_sum128_kernel stores the decrypt mask -- keeps that kernel's budget: no scratch, no spilled VGPRs, at most 128 VGPRs (four
1,024-thread waves per SIMD) and the same LDS, per the code objects inside the built library (tools/kernel_resources.py).  It is a
kernel of its own: the pinned kernels' budgets are checked by their own tests, unedited."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dec_sum128_kernel_budget():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.resources(os.path.join(ROOT, "flashe_amd", "libflashe_hip.so"))
    dec = [r for k, r in res.items() if "prf_dec_sum128_kernel<1024>" in k]
    assert len(dec) == 1, [k for k in res if "sum128" in k]
    r = dec[0]
    assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, r
    assert r["vgpr"] + r["agpr"] <= 128, r
    assert r["max_workgroup"] == 1024, r
    dm = [v for k, v in res.items() if "prf_dmask_sum128_kernel<1024>" in k]
    assert len(dm) == 1 and r["lds_bytes_static"] == dm[0]["lds_bytes_static"] == 133632, (r, dm)
