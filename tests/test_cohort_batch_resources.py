"""CPU test: the three batched instantiations of the cohort chain (prf_chain_cohort_batch_kernel<1024, 5 / 6 / 7>, kernels.hip: a
quantise-and-pack front end on every link) fit the budget that keeps one 1,024-thread workgroup resident per CU beside the 128-KiB AES
tables -- no scratch, no VGPR spills, at most 128 VGPRs, the static LDS of prf_chain_dmask_kernel -- per the code objects inside the built
library (tools/kernel_resources.py)."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    return kernel_resources.resources(os.path.join(ROOT, "flashe_amd", "libflashe_hip.so"))


def test_exactly_the_three_batch_sizes_are_compiled_and_each_fits_the_budget():
    res = _resources()
    hit = {}
    for k, r in res.items():
        m = re.search(r"prf_chain_cohort_batch_kernel<1024, (\d+)>", k)
        if m:
            assert int(m.group(1)) not in hit, k
            hit[int(m.group(1))] = r
    assert sorted(hit) == [5, 6, 7], [k for k in res if "cohort_batch" in k]
    assert len([k for k in res if "prf_chain_cohort_batch_kernel" in k]) == 3
    dm = [v for k, v in res.items() if "prf_chain_dmask_kernel<1024>" in k]
    assert len(dm) == 1
    for bs, r in sorted(hit.items()):
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, (bs, r)
        assert r["vgpr"] + r["agpr"] <= 128, (bs, r)
        assert r["max_workgroup"] == 1024, (bs, r)
        assert r["lds_bytes_static"] == dm[0]["lds_bytes_static"], (bs, r, dm)
