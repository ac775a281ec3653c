"""CPU test: plan_cohort's compact=True rule (FlasheCohort(compact=True), flashe_quantize_encrypt_cohort_u32_dev) -- the chained launch at
the five compiled-in widths from exactly the admission length of the summed compact chain on, whatever the chunking, every other shape
on the fallbacks it takes today with a reason -- and compact=False unchanged.  Touches no device and no library."""
import numpy as np
import pytest

from flashe_amd.block import (cohort_admission_length, compact_cohort_admission_length, compact_cohort_blocks, plan_cohort)

WIDTHS = (16, 20, 23, 24, 32)


class _W:
    def __init__(self, layers):
        self.walking_order = sorted(layers)
        self._weights = dict(layers)


def _layer(n, dtype=np.float32):
    return np.broadcast_to(np.zeros((), dtype), (n,))          # (a shape and a dtype: the planner reads nothing else)


def _cohort(n, C=2, dtype=np.float32):
    head = min(n, 1234)
    return [_W({"a": _layer(head, dtype), "b": _layer(0), "c": _layer(n - head)}) for _ in range(C)]


def _blocks(n, b, J):
    """The count block_of (csrc/kernels.hip) defines: r chunks of d + 1 elements and J - r of d, each cut into blocks of m of its own."""
    m, d, r = 128 // b, n // J, n % J
    return r * -(-(d + 1) // m) + (J - r) * -(-d // m)


@pytest.mark.parametrize("n_jobs", [16, 1, 7])
@pytest.mark.parametrize("cu", [256, 80])
@pytest.mark.parametrize("b", WIDTHS)
def test_compact_chains_from_the_admission_length_on(b, cu, n_jobs):
    need = 2 * 128 * 16 * cu
    n = compact_cohort_admission_length(cu, b, n_jobs)
    assert _blocks(n, b, n_jobs) >= need > _blocks(n - 1, b, n_jobs)
    assert compact_cohort_blocks(n, b, n_jobs) == _blocks(n, b, n_jobs)
    at = plan_cohort(_cohort(n), b, cu, compact=True, n_jobs=n_jobs)
    assert (at.path, at.reason, at.n, at.n_elems) == ("cohort-chain", "", n, n)
    below = plan_cohort(_cohort(n - 1), b, cu, compact=True, n_jobs=n_jobs)
    assert below.path == "staged-chain" and "fill the chip" in below.reason


def test_the_default_chunking_is_the_ciphers():
    from flashe_amd import cipher as cm
    n = compact_cohort_admission_length(80, 20, cm.N_JOBS)
    assert plan_cohort(_cohort(n), 20, 80, compact=True).path == "cohort-chain"
    assert plan_cohort(_cohort(n - 1), 20, 80, compact=True).path == "staged-chain"


def test_every_other_shape_falls_back_with_a_reason():
    cu, J = 80, 16
    n = compact_cohort_admission_length(cu, 16, J) + 1000        # (the longest admission length of the widths below)
    ok = dict(compact=True, n_jobs=J)
    assert plan_cohort(_cohort(n), 20, cu, **ok).path == "cohort-chain"
    for b in (12, 21, 33):
        p = plan_cohort(_cohort(n), b, cu, **ok)
        assert p.path == "staged-chain" and f"int_bits {b}" in p.reason
    p = plan_cohort(_cohort(n), 32, cu, element_bits=12, batch=True, **ok)
    assert (p.path, p.reason) == ("staged-chain", "batched job")
    p = plan_cohort(_cohort(n), 20, cu, mask="single", **ok)
    assert p.path == "staged-chain" and "single mask" in p.reason
    p = plan_cohort(_cohort(n), 20, cu, precompute=True, **ok)
    assert p.path == "per-client" and "precomputed" in p.reason
    p = plan_cohort(_cohort(n, C=129), 20, cu, **ok)
    assert p.path == "staged-chain" and "128 clients" in p.reason
    assert plan_cohort(_cohort(n, C=128), 20, cu, **ok).path == "cohort-chain"
    p = plan_cohort(_cohort(n), 20, cu, chain=False, **ok)
    assert (p.path, p.reason) == ("staged-chain", "FLASHE_CHAIN=0")
    mixed = _cohort(n)
    mixed[1]._weights["a"] = _layer(mixed[1]._weights["a"].shape[0], np.float64)
    p = plan_cohort(mixed, 20, cu, **ok)
    assert p.path == "staged-chain" and "float64 for some clients only" in p.reason
    assert plan_cohort(_cohort(n, dtype=np.float64), 20, cu, **ok).path == "cohort-chain"       # (float64 for all: a shared row)


@pytest.mark.parametrize("b", [16, 20, 23, 64, 65, 128])
def test_compact_false_is_todays_plan(b):
    cu = 80
    for n in (cohort_admission_length(cu) - 1, cohort_admission_length(cu), compact_cohort_admission_length(cu, 16, 16) + 5):
        for kw in ({}, {"mask": "single"}, {"precompute": True}, {"chain": False}, {"batch": True, "element_bits": 4}):
            a = plan_cohort(_cohort(n), b, cu, **kw)
            e = plan_cohort(_cohort(n), b, cu, compact=False, n_jobs=3, **kw)
            assert (a.path, a.reason, a.n, a.n_elems, a.draw_offsets) == (e.path, e.reason, e.n, e.n_elems, e.draw_offsets)
            if kw:
                continue
            if b <= 64:
                assert (a.path, a.reason) == ("staged-chain", "int_bits <= 64")
            elif n < cohort_admission_length(cu):
                assert a.path == "staged-chain" and "fill the chip" in a.reason
            else:
                assert (a.path, a.reason) == ("cohort-chain", "")
