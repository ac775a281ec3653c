"""CPU test: the engine-free planner of FlasheSparseCohort (flashe_amd.block.plan_sparse_cohort) -- the per-layer counts Client.sparsify
keeps, the compact layout and the client-major draws with their 'zzz' slots, the checks that the clients hold one model, every row of
the path table -- and the fact the path table rests on: the arbiter's cost rule answers "single" for strictly increasing lists, so a
sparsifier-fed round never takes the "double" fallback by itself.  Touches no device."""
import numpy as np
import pytest

from flashe_amd.block import PER_CLIENT, SPARSE_COHORT, dynamic_masking_choice, plan_sparse_cohort


class _W:
    def __init__(self, layers, order=None):
        self._weights = dict(layers)
        self.walking_order = list(order) if order is not None else sorted(self._weights)


class _Tensor:
    """A stand-in for a framework tensor: the planner only reads shape and dtype."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = shape, dtype


def _model(dtype=np.float32):
    # a one-value layer, a prime-sized one, one whose sparsity floors to zero entries, a matrix
    return {"a": np.zeros(1, dtype), "b": np.zeros(1013, dtype), "c": np.zeros(99, dtype), "d": np.zeros((30, 40), dtype)}


def test_layout_counts_and_draw_offsets():
    p = plan_sparse_cohort([_model() for _ in range(4)], 0.01, 128)
    assert p.names == ["a", "b", "c", "d"] and p.shapes == [(1,), (1013,), (99,), (30, 40)]
    assert p.sizes == [1, 1013, 99, 1200] and p.starts == [0, 1, 1014, 1113] and p.total == 2313 and p.bits == 12
    assert p.ks == [1, 10, 1, 12]                         # max(1, floor(0.01 * size)): 0.01 * 99 floors to zero, one entry is kept
    assert p.K == 24 and p.compact_starts == [0, 1, 11, 12] and p.n_elems == 25
    assert p.draw_offsets == [0, 25, 50, 75]              # client c's K values, then its 'zzz' draw
    assert p.f64 == [False] * 4 and p.path == SPARSE_COHORT
    # Weights objects and plain dicts, an explicit walking order, NumPy's floor on the product as Sparsifier computes it
    q = plan_sparse_cohort([_W(_model(np.float64), order=["d", "a", "c", "b"]) for _ in range(2)], 0.1, 20)
    assert q.names == ["d", "a", "c", "b"] and q.ks == [120, 1, 9, 101] and q.compact_starts == [0, 120, 121, 130] and q.K == 231
    assert q.f64 == [True] * 4 and q.draw_offsets == [0, 232]
    for s in (0.1, 0.01, 0.3, 1e-7):
        r = plan_sparse_cohort([_model()], s, 128)
        assert r.ks == [max(1, int(np.floor(s * n))) for n in r.sizes]


@pytest.mark.parametrize("bad, word", [
    (lambda: {"w": np.zeros(4, np.float32), "other": np.zeros(2, np.float32)}, "other"),
    (lambda: {"w": np.zeros(4, np.float32)}, "x"),
    (lambda: {"w": np.zeros(5, np.float32), "x": np.zeros(2, np.float32)}, "w"),
    (lambda: {"w": np.zeros((2, 2), np.float32), "x": np.zeros(2, np.float32)}, "w"),
    (lambda: _W({"w": np.zeros(4, np.float32), "x": np.zeros(2, np.float32)}, order=["x", "w"]), "x"),
])
def test_mismatched_clients_are_named(bad, word):
    good = lambda: _W({"w": np.zeros(4, np.float32), "x": np.zeros(2, np.float32)})     # noqa: E731
    with pytest.raises(ValueError) as e:
        plan_sparse_cohort([good(), good(), bad()], 0.1, 128)
    assert "client 2" in str(e.value) and repr(word) in str(e.value)


def test_an_empty_layer_and_an_empty_cohort_are_refused():
    with pytest.raises(ValueError, match="'e' is empty"):
        plan_sparse_cohort([{"w": np.zeros(4, np.float32), "e": np.zeros((0, 3), np.float32)} for _ in range(2)], 0.1, 128)
    with pytest.raises(ValueError):
        plan_sparse_cohort([], 0.1, 128)


def test_every_row_of_the_path_table():
    ws = [_model() for _ in range(3)]
    assert plan_sparse_cohort(ws, 0.1, 128).path == SPARSE_COHORT
    assert plan_sparse_cohort(ws, 0.1, 20, element_bits=12).path == SPARSE_COHORT        # the reference's sparse jobs ship int_bits 20
    assert plan_sparse_cohort([{"w": np.zeros(1, np.float32)}], 0.1, 128).path == SPARSE_COHORT     # no minimum size
    for kw in ({"choice": "double"}, {"batch": True}, {"precompute": True}, {"fuse": False}):
        p = plan_sparse_cohort(ws, 0.1, 128, **kw)
        assert p.path == PER_CLIENT and p.reason, kw
    # one compute class per layer: float64, or float32 / float16 / bfloat16, for all clients
    t = lambda dt: {"a": _Tensor((7,), dt), "b": _Tensor((9, 2), "float64")}             # noqa: E731
    assert plan_sparse_cohort([t("float32"), t("torch.bfloat16"), t("float16")], 0.1, 128).path == SPARSE_COHORT
    assert plan_sparse_cohort([t("float32"), t("float64")], 0.1, 128).path == PER_CLIENT
    assert plan_sparse_cohort([_model(np.float32), _model(np.float64)], 0.1, 128).path == PER_CLIENT
    assert plan_sparse_cohort([_model(np.float64), _model(np.float64)], 0.1, 128).f64 == [True] * 4
    mixed = {"a": np.zeros(3, np.float32), "b": np.zeros(3, np.float64)}                 # mixed INSIDE the model, the same for all
    assert plan_sparse_cohort([dict(mixed), dict(mixed)], 0.1, 128).path == SPARSE_COHORT


def test_strictly_increasing_lists_always_cost_single():
    """single_cost <= double_cost is sum_i |M_i & M_{i+1}| <= sum_i |M_i|: true whenever the lists are sets, which is what a
    sparsifier emits -- identical lists and full-density lists included."""
    g = np.random.Generator(np.random.PCG64(2024))
    for trial in range(300):
        total = int(g.integers(1, 400))
        C = int(g.integers(1, 9))
        kind = trial % 4
        if kind == 0:                                     # every client the same list
            one = np.sort(g.choice(total, size=int(g.integers(1, total + 1)), replace=False))
            masks = [one.copy() for _ in range(C)]
        elif kind == 1:                                   # full density
            masks = [np.arange(total) for _ in range(C)]
        else:
            masks = [np.sort(g.choice(total, size=int(g.integers(1, total + 1)), replace=False)) for _ in range(C)]
        assert all(np.all(m[1:] > m[:-1]) for m in masks)
        assert dynamic_masking_choice([m.tolist() for m in masks], total) == "single", (trial, total, C)
