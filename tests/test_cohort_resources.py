"""CPU test: the cohort instantiation of the summed decrypt-mask chain (prf_chain_cohort_kernel, kernels.hip: a quantising front end on
every link) fits the budget that keeps one 1,024-thread workgroup resident per CU beside the 128-KiB AES tables -- no scratch, no VGPR
spills, at most 128 VGPRs, the static LDS of prf_chain_dmask_kernel -- and the three headline kernels it was kept apart from still report
the figures of the commit before it, per the code objects inside the built library (tools/kernel_resources.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# vgpr, sgpr_spills, lds_bytes_static of the headline kernels as the parent commit's library reported them
PINNED = {
    "prf_chain_kernel<1024, true, false>": (99, 37, 133632),
    "prf_chain_dmask_kernel<1024>": (115, 54, 133632),
    "prf_dmask_sum128_kernel<1024>": (102, 43, 133632),
}


def _resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    return kernel_resources.resources(os.path.join(ROOT, "flashe_amd", "libflashe_hip.so"))


def test_cohort_kernel_budget():
    res = _resources()
    co = [r for k, r in res.items() if "prf_chain_cohort_kernel<1024>" in k]
    assert len(co) == 1, [k for k in res if "cohort" in k]
    r = co[0]
    assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, r
    assert r["vgpr"] + r["agpr"] <= 128, r
    assert r["max_workgroup"] == 1024, r
    dm = [v for k, v in res.items() if "prf_chain_dmask_kernel<1024>" in k]
    assert len(dm) == 1 and r["lds_bytes_static"] == dm[0]["lds_bytes_static"], (r, dm)


def test_headline_kernels_keep_their_figures():
    res = _resources()
    for name, (vgpr, sgpr_spills, lds) in PINNED.items():
        hit = [r for k, r in res.items() if name + "(" in k]
        assert len(hit) == 1, (name, [k for k in res if "prf_chain" in k or "sum128" in k])
        r = hit[0]
        assert (r["vgpr"], r["sgpr_spills"], r["lds_bytes_static"]) == (vgpr, sgpr_spills, lds), (name, r)
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, (name, r)
