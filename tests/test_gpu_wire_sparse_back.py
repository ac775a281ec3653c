"""GPU: the sparse job's way back in one launch (flashe_unpack_sparse_decrypt_unquantize_model_dev; span_prf_small_wire_kernel, stream.hip).
No kernel of the engine goes into an expected value: the packed input is the Python int of a random int_bits-bit aggregate (wire_ref), the
floats are codec_ref's unquantise of the CPU oracle's combine(aggregate, -sparse_minus_mask), compared as float64 BYTES; the output is
filled with 0xFF first and a guard value lies behind it."""
import numpy as np
import pytest

import wire_ref as W
from test_gpu_sparse_small_width import KEY, SPAN, lists, ragged, upload_all

pytestmark = pytest.mark.gpu
ALPHAS = (8.17121, 3e-3, 6.5, 0.7, 41.0, 1.25e-2)
SHAPES = [(1, 1), (3, 1_751), (5, 1_752), (6, 1_753), (64, 3 * 1_752 + 11), (6, 7 * 1_752 + 1)]
CASES = [(b, J, SHAPES[(i + 2 * j) % len(SHAPES)]) for i, b in enumerate((16, 20, 23, 33, 63, 64)) for j, J in enumerate((1, 16, 40))]


def engine(b):
    from flashe_amd.engine import Engine
    return Engine(KEY, b, device=0)


def layers_of(total, sizes=(7, 1, 1744)):
    """(starts, sizes): rows of `sizes` cut short where total is smaller, then the rest: a one-position row, a boundary on the first span edge"""
    out = [min(s, max(total - sum(sizes[:i]), 0)) for i, s in enumerate(sizes)] + [max(total - sum(sizes), 0)]
    out = [s for s in out if s]
    return [int(v) for v in np.cumsum([0] + out[:-1])], out


def packed(eng, agg_h, b):
    return eng.upload(W.int_limbs(W.wire_int(agg_h, b), W.n_limbs_of(len(agg_h), b)))


def run(eng, it, dl, ks, total, J, din, starts, bounds=None):
    """one call over `total` values and a guard, all 0xFF bytes before it: (took, the total + 1 words behind the call)"""
    out = eng.alloc(8 * (total + 1))
    eng.memset_dev(out, 0xFF, out.nbytes)
    table = [(s, None, a, False) for s, a in zip(starts, ALPHAS)]
    took = eng.unpack_sparse_decrypt_unquantize_model_dev(it, dl, ks, total, J, din, table, W.EBITS, W.C, out, bounds=bounds)
    return took, out.download(np.uint64, total + 1)


def check(oracle, res, it, agg_h, locs, J, b, starts, sizes, tag):
    total = len(agg_h)
    dec = oracle.combine(b, agg_h.reshape(total, 1), None, oracle.sparse_minus_mask(KEY, it, locs, total, J, b))[:, 0]
    floats = W.row_floats([int(v) for v in dec], starts, sizes, ALPHAS)
    assert res[0] and int(res[1][total]) == W.GUARD, tag
    assert res[1][:total].tobytes() == floats.tobytes(), tag + (np.flatnonzero(res[1][:total] != floats.view(np.uint64))[:4],)


@pytest.mark.parametrize("b,J,shape", CASES, ids=[f"b{b}-J{J}-C{s[0]}-n{s[1]}" for b, J, s in CASES])
def test_packed_sparse_sum_to_floats(oracle, b, J, shape):
    """Every width class and chunking over the short last span, spans that start mid-limb, fields that straddle limbs or end on a limb edge,
    a partial top limb and the C = 64 table; ragged lists (every position, none, one, fewer than chunks, ...); with and without a handle."""
    (C, total), eng = shape, engine(b)
    rng = np.random.Generator(np.random.PCG64(4300 + b * 100 + J + C))
    ks = ragged(rng, C, total, J)
    locs = lists(rng, total, ks)
    agg_h = rng.integers(0, 2 ** b, total, dtype=np.uint64)
    (starts, sizes), dl, din = layers_of(total), upload_all(eng, locs), packed(eng, agg_h, b)
    for bounds in (None, eng.span_bounds(total, dl, ks)):
        check(oracle, run(eng, 8, dl, ks, total, J, din, starts, bounds), 8, agg_h, locs, J, b, starts, sizes, (b, J, C, total, bounds is not None))


def test_crowded_full_and_empty_spans_two_iters(oracle):
    """40 spans of changing density -- five clients holding every position (more blocks than lanes), 1 %, empty -- over two iters on one
    engine; rows of 1 .. 3 positions across a span edge."""
    b, J, C, n_spans, eng = 20, 16, 6, 40, engine(20)
    total = SPAN * n_spans - 7
    rng = np.random.Generator(np.random.PCG64(4343))
    dens = np.array([[1.0, 1.0, 1.0, 1.0, 1.0, 0.5], [0.01] * 6, [0.0] * 6, [1.0, 0.01, 0.0, 0.2, 0.0, 0.01], [0.3, 0.3, 0.25, 0.02, 0.0, 0.01]])
    p_of_pos = dens[np.repeat(np.arange(n_spans) % 5, SPAN)[:total]]
    locs = [np.flatnonzero(rng.random(total) < p_of_pos[:, c]).astype(np.uint32) for c in range(C)]
    ks = [int(l.size) for l in locs]
    assert sum(int(np.count_nonzero(l < SPAN)) for l in locs) > 1024 * (128 // b)
    (starts, sizes), dl = layers_of(total, (5 * SPAN - 2, 1, 3, 2, 11 * SPAN)), upload_all(eng, locs)
    bnd = eng.span_bounds(total, dl, ks)
    for it in (3, 4):
        agg_h = rng.integers(0, 2 ** b, total, dtype=np.uint64)
        check(oracle, run(eng, it, dl, ks, total, J, packed(eng, agg_h, b), starts, bnd), it, agg_h, locs, J, b, starts, sizes, (it,))


def test_refusals_leave_the_output_alone():
    """More than 64 clients, int_bits 8 and int_bits 128 are declined with nothing written; a bounds handle of other lists is an error."""
    from flashe_amd._lib import FlasheError
    total, J, rng = 1_753, 16, np.random.Generator(np.random.PCG64(43))
    starts, _sizes = layers_of(total)

    def call(b, C, other_bounds):
        eng, ks = engine(b), [5] * C
        dl, din = upload_all(eng, lists(rng, total, ks)), eng.alloc(8 * W.n_limbs_of(total, b))
        bounds = eng.span_bounds(total, upload_all(eng, lists(rng, total, ks)), ks) if other_bounds else None
        return run(eng, 8, dl, ks, total, J, din, starts, bounds)

    for b, C in ((20, 65), (8, 3), (128, 3)):
        took, words = call(b, C, False)
        assert not took and np.all(words == np.uint64(W.GUARD)), (b, C)
    with pytest.raises(FlasheError):
        call(20, 3, True)


@pytest.mark.parametrize("decline", [False, True])
def test_sparse_client_takes_the_packed_sum_in_one_launch(monkeypatch, decline):
    """decrypt_unquantize of a sparse single-mask round under _WIRE_SPARSE_BACK: the PackedVector returns the DeviceVector's layers, as
    bytes, through one call of the new engine method -- and through the staged launches when that call declines."""
    from flashe_amd import block, cipher as cm
    from flashe_amd.engine import PackedVector
    from flashe_amd.weights import Sparsifier, from_big_int
    from test_gpu_wire_python_surface import _W
    monkeypatch.setattr(block, "_WIRE_SPARSE_BACK", True)
    monkeypatch.setattr(cm, "N_JOBS", 16)
    b, sizes, rng = 20, {"a": 3_000, "b": 1, "c": 2_255}, np.random.Generator(np.random.PCG64(7))
    total = sum(sizes.values())
    w = {k: (rng.standard_normal(s) * 0.05).astype(np.float32) for k, s in sizes.items()}
    cl = block.FlasheClient({"quantize": {"int_bits": b, "batch": False, "element_bits": 16, "padding": True, "secure": True},
                             "precompute": {"enable": False}, "mask": "dynamic"})
    cl.create_cipher(0, 1, KEY)
    cl.set_iter_index(1)
    cl.cipher.total = total
    sp = Sparsifier(0.1)
    enc, le, bits, _t = sp.sparsify(w, sorted(sizes))
    mask = np.asarray(from_big_int(enc, le, bits, as_object=False)).astype(np.int64)
    cl.dynamic_masking("single", [mask])
    np.random.seed(3)
    up = cl.quantize_encrypt(_W(dict(w, zzz=np.array([0.0]))), device=True)
    eng = cl.cipher.engine
    agg = block.aggregate_sparse_uploads(eng, [up._weights["a"]], [mask], total, device=True)
    wire = PackedVector.from_int(eng, W.wire_int(agg.to_host()[:, 0], b), total, b)
    cl.shape_dict = dict(sp.shape_dict_used_for_sparsification)
    took, fused = [], eng.unpack_sparse_decrypt_unquantize_model_dev
    monkeypatch.setattr(eng, "unpack_sparse_decrypt_unquantize_model_dev", lambda *a, **kw: took.append(not decline and fused(*a, **kw)) or took[-1])
    res = []
    for v in (agg, wire):
        cl.set_idx_list([0])
        res.append(cl.decrypt_unquantize(_W({"a": v})))
    assert took == [not decline]
    for k in sizes:
        assert res[1]._weights[k].tobytes() == res[0]._weights[k].tobytes(), k
