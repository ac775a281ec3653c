"""GPU: the sparse job's packed wire uploads reduced to the packed dense sum in one launch (flashe_sparse_aggregate_packed_dev).  No kernel
of the engine goes into an expected value: an upload is the Python int of random fields and a zero (wire_ref), the sum the Python int of
NumPy's uint64 arithmetic mod 2^b, compared as limb BYTES; the output is filled with 0xFF first and a guard limb lies behind it."""
import numpy as np
import pytest

import wire_ref as W
from test_gpu_sparse_small_width import KEY, bmask, lists, ragged, upload_all

pytestmark = pytest.mark.gpu
SPAN = 4096
SHAPES = [(1, 1), (3, SPAN - 1), (5, SPAN), (6, SPAN + 1), (64, 3 * SPAN + 11), (6, 7 * SPAN + 1)]


def engine(b):
    from flashe_amd.engine import Engine
    return Engine(KEY, b, device=0)


def make_round(rng, b, total, locs):
    """(every client's upload as limbs -- its values at its locations, then its zero --, the limbs of the expected dense sum)"""
    near = np.uint64(2 ** 64 - 2 ** 8 if b == 64 else 0)      # (b = 64: every other value within 2^8 of 2^64, so the sums wrap)
    vals = [(rng.integers(0, 2 ** 64, len(l), dtype=np.uint64) | near * (np.arange(len(l), dtype=np.uint64) % 2)) & bmask(b) for l in locs]
    zeros = [rng.integers(0, 2 ** 64, dtype=np.uint64) & bmask(b) for _ in locs]
    dense = np.full(total, np.sum(np.array(zeros, dtype=np.uint64)), dtype=np.uint64)
    with np.errstate(over="ignore"):
        for l, v, z in zip(locs, vals, zeros):
            dense[l] += v - z
    ups = [W.int_limbs(W.wire_int(np.append(v, z), b), W.n_limbs_of(len(v) + 1, b)) for v, z in zip(vals, zeros)]
    return ups, W.int_limbs(W.wire_int(dense & bmask(b), b), W.n_limbs_of(total, b))


def run(eng, total, dl, ks, dup, b, bounds=None, out=None):
    """one call over the sum's limbs and a guard limb, all 0xFF bytes before it: (took, the n_limbs + 1 words behind it, their buffer)"""
    out = out or eng.alloc(8 * (W.n_limbs_of(total, b) + 1))
    eng.memset_dev(out, 0xFF, out.nbytes)
    return eng.sparse_aggregate_packed_dev(total, dl, ks, dup, out, bounds=bounds), out.download(np.uint64, W.n_limbs_of(total, b) + 1), out


def check(eng, b, total, locs, rng, tag):
    ups, want = make_round(rng, b, total, locs)
    dl, dup, ks = upload_all(eng, locs), [eng.upload(u) for u in ups], [int(l.size) for l in locs]
    for bounds in (None, eng.span_bounds(total, dl, ks)):
        took, got, _out = run(eng, total, dl, ks, dup, b, bounds)
        assert took and int(got[-1]) == W.GUARD, tag
        assert got[:-1].tobytes() == want.tobytes(), tag + (bounds is not None, np.flatnonzero(got[:-1] != want)[:4])


@pytest.mark.parametrize("shape", SHAPES, ids=[f"C{c}-n{n}" for c, n in SHAPES])
@pytest.mark.parametrize("b", [16, 20, 23, 33, 63, 64])
def test_packed_uploads_to_the_packed_sum(b, shape):
    """total b = 0 and != 0 mod 64, a short last span, a partial top limb, the C = 64 table; ragged lists; with and without a handle."""
    (C, total), eng = shape, engine(b)
    rng = np.random.Generator(np.random.PCG64(4400 + b * 100 + C))
    check(eng, b, total, lists(rng, total, ragged(rng, C, total, 16)), rng, (b, C, total))


@pytest.mark.parametrize("b", [20, 23, 63])
def test_span_edges_from_both_sides(b):
    """One client holds every position, three hold different subsets of {p0 - 4 .. p0 + 3} around both span edges, one holds nothing: the
    halo accumulators and the cut limb are fed from either side."""
    total, eng = 3 * SPAN + 5, engine(b)
    around = [[-4, -3, -2, -1, 0, 1, 2, 3], [-1, 0], [-4, -2, 3], []]
    second = [[-4, -3, -2, -1, 0, 1, 2, 3], [-2], [-3, 1], []]
    locs = [np.arange(total, dtype=np.uint32)] + [np.array([SPAN + d for d in a] + [2 * SPAN + d for d in s], dtype=np.uint32)
                                                  for a, s in zip(around, second)]
    check(eng, b, total, locs, np.random.Generator(np.random.PCG64(44 + b)), (b,))


def test_refusals_leave_the_output_alone():
    """More than 64 clients, int_bits 8 and 128 are declined with nothing written; a handle of other lists is an error; a repeated position
    is reported by the next synchronising call (the err flag of the sparse passes), the guard intact."""
    from flashe_amd._lib import FlasheError
    total, rng = SPAN + 1, np.random.Generator(np.random.PCG64(44))

    def call(b, C, other_bounds=False):
        eng, locs, ks = engine(b), lists(rng, total, [5] * C), [5] * C
        dl, dup = upload_all(eng, locs), [eng.upload(np.zeros(W.n_limbs_of(k + 1, b), dtype=np.uint64)) for k in ks]
        bounds = eng.span_bounds(total, upload_all(eng, lists(rng, total, ks)), ks) if other_bounds else None
        return run(eng, total, dl, ks, dup, b, bounds)

    for b, C in ((20, 65), (8, 3), (128, 3)):
        took, words, _out = call(b, C)
        assert not took and np.all(words == np.uint64(W.GUARD)), (b, C)
    with pytest.raises(FlasheError):
        call(20, 3, other_bounds=True)
    eng = engine(20)
    out = eng.alloc(8 * (W.n_limbs_of(total, 20) + 1))
    with pytest.raises(FlasheError):
        run(eng, total, [eng.upload(np.array([3, 3, 9], dtype=np.uint32))], [3], [eng.upload(np.zeros(2, dtype=np.uint64))], 20, out=out)
    assert int(out.download(np.uint64, W.n_limbs_of(total, 20) + 1)[-1]) == W.GUARD


@pytest.mark.parametrize("how", ["fused", "declined", "unsorted"])
def test_aggregate_sparse_uploads_takes_packed_vectors(monkeypatch, how):
    """aggregate_sparse_uploads of PackedVectors returns, as limbs, the packed form of what it returns for the same uploads as
    DeviceVectors: through the one launch, through the staged passes when it declines or a host list is not strictly increasing (the
    launch is then not asked); mixed operands and PackedVectors of another length or width are refused."""
    from flashe_amd import block
    from flashe_amd.engine import DeviceVector, PackedVector
    b, total, eng, rng = 20, SPAN + 77, engine(20), np.random.Generator(np.random.PCG64(45))
    locs = lists(rng, total, [total, 0, 300])
    if how == "unsorted":
        locs[2] = rng.permutation(locs[2])
    fields = [rng.integers(0, 2 ** b, l.size + 1, dtype=np.uint64) for l in locs]
    pvs = [PackedVector.from_int(eng, W.wire_int(f, b), len(f), b) for f in fields]
    dvs = [DeviceVector.from_host(eng, f) for f in fields]
    monkeypatch.setattr(block, "_WIRE_SPARSE_AGG", True)
    took, fused = [], eng.sparse_aggregate_packed_dev
    monkeypatch.setattr(eng, "sparse_aggregate_packed_dev", lambda *a, **kw: took.append(how == "fused" and fused(*a, **kw)) or took[-1])
    dense = block.aggregate_sparse_uploads(eng, dvs, locs, total, device=False)[:, 0]
    res = block.aggregate_sparse_uploads(eng, pvs, locs, total)
    assert took == {"fused": [True], "declined": [False], "unsorted": []}[how] and res.path == ("fused" if how == "fused" else "staged")
    assert (len(res), res.bits) == (total, b) and res.to_int() == W.wire_int(dense, b) == block.aggregate_sparse_uploads(eng, pvs, locs, total, device=False)
    with pytest.raises(TypeError):
        block.aggregate_sparse_uploads(eng, [pvs[0], dvs[1], pvs[2]], locs, total)
    for bad in (PackedVector(eng, len(fields[2]) + 1, b), PackedVector(eng, len(fields[2]), 23)):
        with pytest.raises(ValueError):
            block.aggregate_sparse_uploads(eng, pvs[:2] + [bad], locs, total)
