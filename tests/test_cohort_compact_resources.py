"""CPU test: the five instantiations of the compact cohort chain (prf_small_cohort_kernel<B>, kernels.hip: the quantising front end on the
summed compact chain at a compile-time width) fit the budget that keeps one 1,024-thread workgroup resident per CU beside the AES tables --
no scratch, no VGPR spills, at most 128 VGPRs -- and the five instantiations of prf_small_chain_kernel whose body they share still report
the figures of the commit before, per the code objects inside the built library (tools/kernel_resources.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WIDTHS = (16, 20, 23, 24, 32)
# vgpr, sgpr_spills of prf_small_chain_kernel<true, unsigned int, B> as the parent commit's library reported them
PINNED = {16: (122, 90), 20: (114, 97), 23: (110, 98), 24: (110, 93), 32: (106, 98)}


def _resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    return kernel_resources.resources(os.path.join(ROOT, "flashe_amd", "libflashe_hip.so"))


def test_compact_cohort_kernels_fit_the_budget():
    res = _resources()
    co = {k: r for k, r in res.items() if "prf_small_cohort_kernel<" in k}
    assert len(co) == 5, sorted(co)
    for b in WIDTHS:
        hit = [r for k, r in co.items() if f"prf_small_cohort_kernel<{b}>(" in k]
        assert len(hit) == 1, (b, sorted(co))
        r = hit[0]
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, (b, r)
        assert r["vgpr"] + r["agpr"] <= 128, (b, r)
        assert r["max_workgroup"] == 1024, (b, r)


def test_the_compact_chain_keeps_its_figures():
    res = _resources()
    for b, (vgpr, sgpr_spills) in PINNED.items():
        hit = [r for k, r in res.items() if f"prf_small_chain_kernel<true, unsigned int, {b}>(" in k]
        assert len(hit) == 1, (b, [k for k in res if "prf_small_chain_kernel" in k])
        r = hit[0]
        assert (r["vgpr"], r["sgpr_spills"]) == (vgpr, sgpr_spills), (b, r)
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, (b, r)
