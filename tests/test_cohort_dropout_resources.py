"""CPU test: the four instantiations of the chain body for a cohort with dropped-out clients (GAPS in prf_chain_body.inc:
prf_chain_cohort_runs_kernel<1024> and prf_chain_cohort_batch_runs_kernel<1024, 5 / 6 / 7>, kernels.hip) fit the budget that keeps one
1,024-thread workgroup resident per CU beside the 128-KiB AES tables -- no scratch, no VGPR spills, at most 128 VGPRs, the 133,632 bytes of
static LDS of the other chain kernels -- per the code objects inside the built library (tools/kernel_resources.py).  The one-run kernels
they were kept apart from are pinned by tests/test_cohort_resources.py and tests/test_cohort_batch_resources.py."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["prf_chain_cohort_runs_kernel<1024>", "prf_chain_cohort_batch_runs_kernel<1024, 5>", "prf_chain_cohort_batch_runs_kernel<1024, 6>",
           "prf_chain_cohort_batch_runs_kernel<1024, 7>"]
LDS_BYTES = 133632


@pytest.fixture(scope="module")
def resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.resources(os.path.join(ROOT, "flashe_amd", "libflashe_hip.so"))
    return {kernel_resources.norm(k): v for k, v in res.items()}, kernel_resources.norm


@pytest.mark.parametrize("name", KERNELS)
def test_the_dropout_kernels_fit_the_chain_budget(resources, name):
    res, norm = resources
    hit = [r for k, r in res.items() if norm(name) + "(" in k]
    assert len(hit) == 1, (name, [k for k in res if "runs_kernel" in k])
    r = hit[0]
    assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, r
    assert r["vgpr"] + r["agpr"] <= 128, r
    assert r["lds_bytes_static"] == LDS_BYTES, r
    assert r["max_workgroup"] == 1024, r


def test_the_one_run_kernels_share_that_lds_figure(resources):
    res, norm = resources
    for name in ("prf_chain_cohort_kernel<1024>", "prf_chain_cohort_batch_kernel<1024, 6>", "prf_chain_dmask_kernel<1024>"):
        hit = [r for k, r in res.items() if norm(name) + "(" in k]
        assert len(hit) == 1 and hit[0]["lds_bytes_static"] == LDS_BYTES, (name, hit)
