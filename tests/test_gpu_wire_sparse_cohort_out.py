"""GPU: a sparse cohort's uploads from the floats straight to their packed wire form (flashe_quantize_encrypt_pack_sparse_cohort_dev,
prf_small_pack_cohort_kernel).  The expected limbs hold no kernel of the engine: per client codec_ref's NumPy quantiser, the CPU oracle's
single-mask encrypt with the same key, iter, index and n_jobs, the quantised 'zzz' value appended, packed with Python integers
(wire_ref.wire_int).  Every limb of every upload, every zeros[c] and the limbs around the uploads are compared."""
import numpy as np
import pytest

import codec_ref as R
from wire_ref import EBITS, GUARD, IT, KEY, int_limbs, n_limbs_of, tiles, wire_int

pytestmark = pytest.mark.gpu

WIDTHS = (16, 20, 23, 33, 63, 64)                    # m = 8, 6, 5, 3, 2, 2; the top limb partial or whole
ENOTSUP_CLIENTS = 193                                # one more than the launch's prefix table holds


def _shapes(m):
    """name -> (C, K, n_jobs, layer sizes): the smallest shapes that reach each branch of the kernel at m elements per block."""
    T = 64 * m
    return {"one-ragged-block": (1, 1, 1, (1,)), "one-whole-tile": (1, T, 1, (T,)), "tile-edge": (1, T + 1, 1, (T + 1,)),
            "three-layers": (3, 3 * T + 17, 1, (5, T, 2 * T + 12)), "chunk-ends": (3, 1000, 7, (1000,)), "most-clients": (64, 130, 2, (130,))}


def _run(eng, orc, b, C, K, n_jobs, sizes, idx, storage="float32", shift_row=None, z64=True):
    """One call against the reference; returns what the binding returned (False: declined, every output still holds its pattern)."""
    alphas = (8.17121, 3e-3, 6.5)
    spec = [(storage, alphas[l % 3], (-0.25 * alphas[l % 3] if l == shift_row else None), False, False, s) for l, s in enumerate(sizes)]
    model = R.cohort_model(spec, C, seed=b + K)
    u = np.empty(C * (K + 1))
    for c in range(C):
        u[c * (K + 1):c * (K + 1) + K] = model.u[c * K:(c + 1) * K]
        u[c * (K + 1) + K] = (0.0, R.ONE_BELOW, 0.5)[c % 3]
    zzz = [(0.0, 1.0, -1.0, 0.3, -7.0, 2.5)[c % 6] for c in range(C)]
    bufs = [[eng.upload(x) for x in held] for held in model.storage]
    n_limbs = n_limbs_of(K + 1, b)
    stride = n_limbs + 1                               # (a gap limb between the uploads: cleared; the limb behind the last one: untouched)
    out, dz = eng.alloc(8 * (C * stride + 1)), eng.alloc(8 * C + 16)
    eng.memset_dev(out, 0xFF, out.nbytes)
    eng.memset_dev(dz, 0xFF, dz.nbytes)
    du = eng.upload(u)
    ok = eng.quantize_encrypt_pack_sparse_cohort_dev(IT, idx, K, n_jobs, model.rows, [[d.ptr for d in row] for row in bufs], [model.dts] * C, EBITS,
                                                     du, K + 1, zzz, z64, out, stride, dz)
    got, got_z = out.download(np.uint64, C * stride + 1), dz.download(np.uint64, C)
    if not ok:
        assert (got == GUARD).all() and (got_z == GUARD).all(), "a refused call wrote an output"
        return False
    mask = (1 << b) - 1
    for c, q in enumerate(R.cohort_plaintexts(model, EBITS)):
        ct = orc.limbs_to_ints(orc.encrypt(KEY, IT, idx[c], "single", n_jobs, b, q.astype(np.uint64) & np.uint64(mask)))
        z = int(R.ref_quantize(np.array([zzz[c]], np.float64 if z64 else np.float32), 1.0, EBITS, u[c * (K + 1) + K:(c + 1) * (K + 1)])[0])
        want = int_limbs(wire_int(list(ct) + [z], b), n_limbs)
        mine = got[c * stride:c * stride + n_limbs]
        assert mine.tobytes() == want.tobytes(), (b, C, K, n_jobs, c, np.flatnonzero(mine != want)[:4])
        assert int(got_z[c]) == z and int(got[c * stride + n_limbs]) == (GUARD if c == C - 1 else 0), (b, c)
    return True


@pytest.fixture(scope="module")
def engines():
    from flashe_amd.engine import Engine
    made = {}
    yield lambda b: made.setdefault(b, Engine(KEY, b, device=0))
    for eng in made.values():
        eng.close()


@pytest.mark.parametrize("shape", list(_shapes(2)))
@pytest.mark.parametrize("b", WIDTHS)
def test_packed_uploads_equal_the_reference(engines, oracle, b, shape):
    m = 128 // b
    C, K, n_jobs, sizes = _shapes(m)[shape]
    ts = tiles(K, n_jobs, m)                           # the shapes reach what they are here for, on the inputs alone
    if shape == "three-layers":
        assert any(not rg and 5 + 64 * m <= e0 for e0, e1, rg in ts) and any(not rg and e0 < 5 + 64 * m < e1 for e0, e1, rg in ts)
    if shape in ("one-ragged-block", "tile-edge", "chunk-ends"):
        assert any(rg for _e0, _e1, rg in ts)
    assert _run(engines(b), oracle, b, C, K, n_jobs, sizes, list(range(5, 5 + C)), z64=b % 2 == 0)


@pytest.mark.parametrize("kw", [{"storage": "float64"}, {"shift_row": 1}, {"idx": [9, 4_000_000_000, 0]}], ids=["float64", "shift", "any-indices"])
def test_float64_layers_the_shift_and_any_indices(engines, oracle, kw):
    C, K, n_jobs, sizes = _shapes(6)["three-layers"]
    kw = dict(kw)
    assert _run(engines(20), oracle, 20, C, K, n_jobs, sizes, kw.pop("idx", [5, 6, 7]), **kw)


@pytest.mark.parametrize("b,C", [(15, 2), (65, 2), (20, ENOTSUP_CLIENTS)])
def test_refusals_write_nothing(engines, oracle, b, C):
    assert _run(engines(b), oracle, b, C, 13, 2, (13,), list(range(C))) is False


def _args(b):
    return {"quantize": {"int_bits": b, "batch": False, "element_bits": 16, "padding": True, "secure": True},
            "precompute": {"enable": False, "num_params": 11}, "mask": "dynamic"}


@pytest.mark.parametrize("declined", [False, True], ids=["fused", "declined"])
@pytest.mark.parametrize("b", [20, 40])
def test_cohort_round(monkeypatch, b, declined):
    """FlasheSparseCohort.quantize_encrypt(packed="fused") against packed=False on the same seeds: 3 clients, K = 401 over two layers."""
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheSparseCohort
    from flashe_amd.engine import Engine
    monkeypatch.setattr(cm, "N_JOBS", 16)
    if declined:
        monkeypatch.setattr(Engine, "quantize_encrypt_pack_sparse_cohort_dev", lambda self, *a, **k: False)
    sizes, names = (1500, 2517), ["l00", "l01"]
    g = np.random.Generator(np.random.PCG64(b))
    models = [{k: (g.standard_normal(s) * 0.05).astype(np.float32) for k, s in zip(names, sizes)} for _ in range(3)]

    def one_round(packed):
        co = FlasheSparseCohort(_args(b), first_idx=0, n_local=3, num_clients=3, prp_seed=KEY, sparsity=0.1)
        co.set_iter_index(1)
        co.sparsify([dict(m) for m in models], names)
        assert co.dynamic_masking() == "single"
        np.random.seed(77)
        up = co.quantize_encrypt(packed=packed)
        back = co.decrypt_unquantize()
        return up, [np.asarray(back._weights[k]).tobytes() for k in names]

    plain, plain_floats = one_round(False)
    up, floats = one_round("fused")
    ints = lambda dv: [int(v) for v in dv.to_host().reshape(-1)]
    assert [u.to_int() for u in up.uploads] == [wire_int(ints(u), b) for u in plain.uploads]
    assert up.aggregate.to_int() == wire_int(ints(plain.aggregate), b) and floats == plain_floats
    if declined:
        assert up.front_end == plain.front_end and {u.path for u in up.uploads} == {"staged"}
    else:                                              # the packed reduce read the zeros from limb 0 of every upload: nothing was downloaded
        assert up.front_end == "wire" and {u.path for u in up.uploads} == {"fused"} and up.aggregate.path == "fused"
