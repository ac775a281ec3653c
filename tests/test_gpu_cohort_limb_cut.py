"""GPU: a SHORT one-limb cohort as one cut chained launch (flashe_quantize_encrypt_cohort_cut_u64_dev, prf_limb_cohort_cut_kernel<2 | 3> +
cohort_cut_combine_u64_kernel; FlasheCohort(one_limb=True, cut=True)).  ABI level on two CUs, where 32 waves make vectors of a few tiles
cut: every ciphertext against the per-client path (flashe_quantize_encrypt_tensors_dev with that client's cipher index and the same
draws) and the sum against flashe_aggregate_elem_dev of those, whole arrays, the words behind every output and the scratch poisoned
beforehand; the refusals with the outputs untouched; the class against the same cohort without cut=.  Everything is bit-exact."""
import numpy as np
import pytest

from test_gpu_cohort import KEY, _W, _args, _host_models

pytestmark = pytest.mark.gpu

POISON = np.uint64(0xA5A5A5A5A5A5A5A5)
GAPPED = [0, 1, 2, 3, 5, 6, 7, 8, 9, 11, 12, 13, 14]
COHORTS = {"12 clients, 3 pieces": list(range(5, 17)), "3 clients, 1 piece": [5, 6, 7], "3 runs": GAPPED}
IT = 3


@pytest.fixture(scope="module")
def E():
    from flashe_amd import engine
    return engine


def _engine(E, b):
    eng = E.Engine(KEY, b, device=0)
    eng.set_cu_limit(2)
    return eng


def _poisoned(eng, nbytes):
    d = eng.alloc(nbytes + 16)
    eng.memset_dev(d, 0xA5, nbytes + 16)
    return d


def _case(E, eng, bits, J, n, idx):
    """Three rows (the second float64, its end inside a half tile; rows of a one-value model are empty), every client's sources and draws,
    and the reference: each client's own fused step at its cipher index, and the element-wise sum of those."""
    from flashe_amd import _lib
    C = len(idx)
    starts, alphas, codes = [0, n // 3, n - n // 4], [0.37, 2.5, 8.17121], [_lib.TENSOR_F32, _lib.TENSOR_F64, _lib.TENSOR_F32]
    sizes = [starts[1], starts[2] - starts[1], n - starts[2]]
    rows = [(starts[li], None, alphas[li], 0.0, codes[li], 0) for li in range(3)]
    g = np.random.Generator(np.random.PCG64(1000 * bits + 10 * J + C))
    u = g.random(C * n)
    u[::5], u[1::5] = 0.0, 1.0 - 2.0 ** -53
    du = eng.upload(u)
    srcs, keep, refs = [], [], []
    for c in range(C):
        xs = [(g.standard_normal(s) * alphas[li]).astype(np.float64 if li == 1 else np.float32) for li, s in enumerate(sizes)]
        ds = [eng.upload(x) for x in xs]
        keep += ds
        srcs.append([d.ptr for d in ds])
        ref = eng.alloc_vec(n)
        trows = [(starts[li], ds[li].ptr, alphas[li], 0.0, codes[li], 0) for li in range(3) if sizes[li]]
        eng.quantize_encrypt_tensors_dev(IT, idx[c], E.SCHEME_DOUBLE, n, J, 0, n, trows, bits, E.DeviceBufferView(du, 8 * c * n, 8 * n), ref)
        refs.append(ref)
    agg = eng.alloc_vec(n)
    eng.aggregate_elem_dev(refs, n, agg)
    want = [r.download(np.uint64, n).copy() for r in refs] + [agg.download(np.uint64, n).copy()]
    return rows, srcs, [codes] * C, du, want, keep


def _launch(eng, bits, J, n, idx, rows, srcs, dts, du, scratch):
    """The launch into poisoned outputs: (its answer, every output as n + 2 words)."""
    outs = [_poisoned(eng, 8 * n) for _ in range(len(idx) + 1)]
    ok = eng.quantize_encrypt_cohort_cut_u64_dev(IT, idx, n, J, rows, srcs, dts, bits, du, outs[:-1], outs[-1], scratch)
    return ok, [d.download(np.uint64, n + 2).copy() for d in outs]


@pytest.mark.parametrize("who", COHORTS)
@pytest.mark.parametrize("n", [1, 15, 383, 1000])
@pytest.mark.parametrize("J", [1, 16])
@pytest.mark.parametrize("b", [33, 42, 43, 64])
def test_the_cut_launch_is_every_clients_own_step_and_their_sum(E, b, J, n, who):
    from flashe_amd.block import cohort_cut_items, cohort_cut_pieces
    idx, bits = COHORTS[who], b - 4
    eng = _engine(E, b)
    parts, begins = eng.cohort_cut_pieces_u64(idx, n, J)
    assert begins == cohort_cut_pieces(idx, cohort_cut_items(n, b, J, True), 2) and parts == len(begins) - 1
    assert parts == (1 if len(idx) == 3 else 3)
    rows, srcs, dts, du, want, keep = _case(E, eng, bits, J, n, idx)
    scratch = _poisoned(eng, 8 * parts * n) if parts > 1 else None           # (one piece: a NULL scratch is accepted)
    ok, got = _launch(eng, bits, J, n, idx, rows, srcs, dts, du, scratch)
    assert ok, "the cut one-limb cohort launch declined the shape"
    for c, (g, w) in enumerate(zip(got, want)):
        bad = np.flatnonzero(g[:n] != w)
        assert bad.size == 0, ("sum" if c == len(idx) else ("client", c), bad[:6], g[bad[:6]], w[bad[:6]], bad.size)
        assert (g[n:] == POISON).all(), ("the words behind output", c)
    if scratch is not None:
        assert (scratch.download(np.uint64, parts * n + 2)[parts * n:] == POISON).all()
    del keep


@pytest.mark.parametrize("what", ["int_bits 32", "int_bits 128", "17 runs", "unsorted idx", "NULL scratch", "misaligned scratch"])
def test_refusals_leave_every_output_untouched(E, what):
    b, n, J, idx, elem_bytes = 40, 383, 16, list(range(12)), 8
    if what.startswith("int_bits"):
        b = int(what.split()[1])
        elem_bytes = 16 if b > 64 else 8
    elif what == "17 runs":
        idx = list(range(0, 34, 2))
    elif what == "unsorted idx":
        idx = [0, 1, 3, 2] + list(range(4, 12))
    eng = _engine(E, b)
    from flashe_amd import _lib
    x, du = eng.upload(np.zeros(n, np.float32)), eng.upload(np.zeros(len(idx) * n))
    rows, srcs, dts = [(0, None, 1.0, 0.0, _lib.TENSOR_F32, 0)], [[x.ptr]] * len(idx), [[_lib.TENSOR_F32]] * len(idx)
    whole = _poisoned(eng, 16 * 16 * n + 16)
    scratch = {"NULL scratch": None, "misaligned scratch": E.DeviceBufferView(whole, 8, 16 * 16 * n)}.get(what, whole)
    outs = [_poisoned(eng, elem_bytes * n) for _ in range(len(idx) + 1)]
    call = lambda: eng.quantize_encrypt_cohort_cut_u64_dev(IT, idx, n, J, rows, srcs, dts, min(b, 64) - 8, du, outs[:-1], outs[-1], scratch)      # noqa: E731
    if what in ("int_bits 32", "int_bits 128", "17 runs"):
        assert call() is False
    else:
        with pytest.raises(E.FlasheError) as ei:
            call()
        assert ei.value.code == -22
    for d in outs + [whole]:
        assert (d.download(np.uint64) == POISON).all()


@pytest.mark.parametrize("present", [None, GAPPED[:11]], ids=["everyone", "three runs"])
def test_the_cohort_class_runs_cut_chain_with_the_staged_forms_bytes(present):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheCohort
    cm.N_JOBS = 16
    C, b, eb = 15, 40, 32
    models = _host_models(C, [1, 333, 0, 667], 7)
    ws = [models[p] for p in (range(C) if present is None else present)]
    rounds = {}
    for cut in (True, False):
        co = FlasheCohort(_args(b, eb), first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, one_limb=True, cut=cut)
        for it in (0, 1):
            co.set_iter_index(it)
            np.random.seed(5)
            up = co.quantize_encrypt([_W(dict(m)) for m in ws], normalize=True, present=present)
            assert up.path == ("cut-chain" if cut else "staged-chain") and co.lead._cohort_mask is None
            new = co.decrypt_unquantize(unnormalize=True)
            rounds[cut, it] = ([np.asarray(v.to_host(), dtype=np.uint64).tobytes() for v in up.ciphertexts + [up.partial_sum]],
                               [np.asarray(new._weights[k], dtype=np.float64).tobytes() for k in new.walking_order])
    assert rounds[True, 0] == rounds[False, 0] and rounds[True, 1] == rounds[False, 1]
    assert rounds[True, 0][0] != rounds[True, 1][0]
