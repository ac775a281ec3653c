"""CPU test: plan_cohort's limb_cut=True rule (FlasheCohort(one_limb=True, cut=True), flashe_quantize_encrypt_cohort_cut_u64_dev) -- a one-limb
cohort whose only obstacle is the length rule plans "cut-chain" with the mirror's pieces, in one run or several; every other shape keeps
its path and reason; limb_cut=False, the default, changes no plan.  Touches no device and no library."""
import numpy as np
import pytest

from flashe_amd.block import cohort_cut_items, cohort_cut_pieces, compact_cohort_admission_length, plan_cohort
from test_cohort_batch_planner import _W, _layer

CU = 80
GAPPED = [0, 1, 2, 3, 5, 6, 7, 8, 9, 11, 12, 13, 14]


def _ws(n, C=12, dtype=np.float32):
    head = min(n, 1234)
    return [_W({"a": _layer(head, dtype), "b": _layer(0), "c": _layer(n - head)}) for _ in range(C)]


@pytest.mark.parametrize("n_jobs", [1, 16])
@pytest.mark.parametrize("b", [33, 42, 43, 64])
def test_cut_chain_below_the_admission_length_and_cohort_chain_at_it(b, n_jobs):
    ok = dict(one_limb=True, cut=True, limb_cut=True, n_jobs=n_jobs)
    n = compact_cohort_admission_length(CU, b, n_jobs)
    at = plan_cohort(_ws(n), b, CU, **ok)
    assert (at.path, at.reason, at.parts) == ("cohort-chain", "", 1)
    for short, present in ((n - 1, None), (61706, None), (1, None), (61706, GAPPED)):
        ws = _ws(short, C=12 if present is None else len(present))
        p = plan_cohort(ws, b, CU, present=present, **ok)
        begins = cohort_cut_pieces(range(12) if present is None else present, cohort_cut_items(short, b, n_jobs, True), CU)
        assert (p.path, p.reason, p.parts) == ("cut-chain", "", len(begins) - 1), (short, present)
    assert plan_cohort(_ws(61706), b, CU, **ok).parts == 3 and plan_cohort(_ws(61706, C=13), b, CU, present=GAPPED, **ok).parts == 3
    assert plan_cohort(_ws(n - 1), b, CU, **ok).parts == 1


@pytest.mark.parametrize("b", [33, 64])
def test_the_other_obstacles_keep_their_reasons(b):
    ok = dict(one_limb=True, cut=True, limb_cut=True, n_jobs=16)
    n = 61706
    mixed = _ws(n)
    mixed[1]._weights["a"] = _layer(mixed[1]._weights["a"].shape[0], np.float64)
    p = plan_cohort(mixed, b, CU, **ok)
    assert p.path == "staged-chain" and "float64 for some clients only" in p.reason
    p = plan_cohort(_ws(n, C=17), b, CU, present=list(range(0, 34, 2)), **ok)
    assert p.path == "staged-chain" and "17 runs" in p.reason and "at most 16 runs" in p.reason
    assert plan_cohort(_ws(n, C=16), b, CU, present=list(range(0, 32, 2)), **ok).path == "cut-chain"
    p = plan_cohort(_ws(n), b, CU, batch=True, element_bits=8, **ok)
    assert (p.path, p.reason) == ("staged-chain", "batched job")
    p = plan_cohort(_ws(n), b, CU, mask="single", **ok)
    assert p.path == "staged-chain" and "single mask" in p.reason
    p = plan_cohort(_ws(n, C=129), b, CU, **ok)
    assert (p.path, p.reason) == ("staged-chain", "more than 128 clients")


@pytest.mark.parametrize("b", [20, 33, 40, 64, 128])
def test_limb_cut_false_is_the_plan_without_the_keyword(b):
    for n in (1, 61706, compact_cohort_admission_length(CU, min(b, 64), 16)):
        for kw in ({}, {"cut": True}, {"cut": True, "cut_any": True}, {"cut": True, "present": GAPPED}, {"mask": "single"}):
            for one_limb in (False, True):
                ws = _ws(n, C=13 if "present" in kw else 12)
                a = plan_cohort(ws, b, CU, one_limb=one_limb, **kw)
                assert vars(a) == vars(plan_cohort(ws, b, CU, one_limb=one_limb, limb_cut=False, **kw)), (b, n, kw)
                if one_limb and 33 <= b <= 64 and n == 61706:
                    assert a.path == "staged-chain"
                if not (one_limb and 33 <= b <= 64):       # other widths, or no one_limb: the keyword changes nothing either way
                    assert vars(a) == vars(plan_cohort(ws, b, CU, one_limb=one_limb, limb_cut=True, **kw)), (b, n, kw)
