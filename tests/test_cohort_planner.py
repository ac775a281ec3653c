"""CPU test: the engine-free planner of FlasheCohort (flashe_amd.block.plan_cohort) -- the checks that the clients' Weights describe one
model, the layout of the shared layer table and of the client-major draws, and the choice of path for every shape the chained cohort
launch declines, on either side of its admission length for two CU counts.  Touches no device."""
import numpy as np
import pytest

from flashe_amd.block import COHORT_CHAIN, PER_CLIENT, STAGED_CHAIN, cohort_admission_length, plan_cohort


class _W:
    def __init__(self, layers, order=None):
        self._weights = dict(layers)
        self.walking_order = list(order) if order is not None else sorted(self._weights)


class _Tensor:
    """A stand-in for a framework tensor: the planner only reads shape and dtype."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = shape, dtype


def _model(n, dtype="float32"):
    """Three layers of n values in all: a prime-sized one, an empty one and the rest (shapes only: nothing is read)."""
    return {"a": _Tensor((7,), dtype), "b": _Tensor((0, 3), dtype), "c": _Tensor((n - 7,), dtype)}


def _plan(ws, **kw):
    args = dict(int_bits=128, cu_count=256, element_bits=16, batch=False, mask="double", num_clients=len(ws))
    args.update(kw)
    return plan_cohort(ws, **args)


def test_layout_and_draw_offsets():
    ws = [_W({"w": np.zeros((3, 4), np.float32), "b": np.zeros(5, np.float64), "e": np.zeros((0,), np.float32)}) for _ in range(4)]
    p = _plan(ws)
    assert p.names == ["b", "e", "w"] and p.shapes == [(5,), (0,), (3, 4)]
    assert p.sizes == [5, 0, 12] and p.starts == [0, 5, 5] and p.n == 17 and p.n_elems == 17
    assert p.draw_offsets == [c * 17 for c in range(4)]
    assert p.path == STAGED_CHAIN                       # far too short to fill a chip


def test_batched_element_count():
    ws = [_W({"w": np.zeros(11, np.float32), "x": np.zeros(3, np.float32)}) for _ in range(3)]
    p = _plan(ws, batch=True)                           # field = 16 + 2 bits, 7 values per 128-bit element
    assert p.n == 14 and p.n_elems == 2 + 1 and p.draw_offsets == [0, 14, 28] and p.path == STAGED_CHAIN


@pytest.mark.parametrize("bad, word", [
    (lambda: _W({"w": np.zeros(4, np.float32), "other": np.zeros(2, np.float32)}), "other"),
    (lambda: _W({"w": np.zeros(4, np.float32)}), "x"),
    (lambda: _W({"w": np.zeros(5, np.float32), "x": np.zeros(2, np.float32)}), "w"),
    (lambda: _W({"w": np.zeros((2, 2), np.float32), "x": np.zeros(2, np.float32)}), "w"),
    (lambda: _W({"w": np.zeros(4, np.float32), "x": np.zeros(2, np.float32)}, order=["x", "w"]), "x"),
])
def test_mismatched_clients_are_named(bad, word):
    good = lambda: _W({"w": np.zeros(4, np.float32), "x": np.zeros(2, np.float32)})     # noqa: E731
    with pytest.raises(ValueError) as e:
        _plan([good(), good(), bad()])
    assert "client 2" in str(e.value) and repr(word) in str(e.value)


def test_sparse_weights_are_refused():
    ws = [_W({"w": np.zeros(4, np.float32), "zzz": np.zeros(1)}) for _ in range(2)]
    with pytest.raises(TypeError):
        _plan(ws)
    with pytest.raises(TypeError):
        _plan([_W({"w": np.zeros(4, np.float32)})], location_masks=True)
    with pytest.raises(ValueError):
        _plan([])


@pytest.mark.parametrize("cus", [256, 80])
def test_admission_length_for_two_cu_counts(cus):
    """launch_prf_batch_sum's rule: two whole 256-element tiles per wave, 16 waves per CU."""
    n = cohort_admission_length(cus)
    assert (n + 255) // 256 == 2 * 16 * cus and (n - 1 + 255) // 256 == 2 * 16 * cus - 1
    assert _plan([_W(_model(n)) for _ in range(2)], cu_count=cus).path == COHORT_CHAIN
    assert _plan([_W(_model(n - 1)) for _ in range(2)], cu_count=cus).path == STAGED_CHAIN
    if cus == 80:
        assert _plan([_W(_model(n)) for _ in range(2)], cu_count=256).path == STAGED_CHAIN


def test_declining_shapes_fall_back():
    n = cohort_admission_length(256)
    ws = [_W(_model(n)) for _ in range(3)]
    assert _plan(ws).path == COHORT_CHAIN
    assert _plan(ws, int_bits=64).path == STAGED_CHAIN
    assert _plan(ws, int_bits=20, element_bits=12).path == STAGED_CHAIN
    assert _plan(ws, batch=True).path == STAGED_CHAIN
    assert _plan(ws, mask="single").path == STAGED_CHAIN
    assert _plan(ws, chain=False).path == STAGED_CHAIN
    assert _plan(ws, precompute=True).path == PER_CLIENT
    assert _plan(ws, mask="dynamic").path == PER_CLIENT
    one = _W(_model(n))
    assert _plan([one] * 128, num_clients=128).path == COHORT_CHAIN
    assert _plan([one] * 129, num_clients=129).path == STAGED_CHAIN
    # a cohort inside a larger federation still chains; a layer that is float64 for one client only does not
    assert _plan(ws, num_clients=10).path == COHORT_CHAIN
    assert _plan([_W(_model(n)), _W(_model(n, "float64"))]).path == STAGED_CHAIN
    assert _plan([_W(_model(n, "float64")), _W(_model(n, "float64"))]).path == COHORT_CHAIN
    assert _plan([_W(_model(n, "torch.bfloat16")), _W(_model(n, "float16")), _W(_model(n))]).path == COHORT_CHAIN
