"""GPU: a SHORT cohort in which clients DROPPED OUT, and a short BATCHED cohort, as one cut chained launch from the floats
(FlasheCohort(cut="any"): flashe_quantize_encrypt_cohort_cut_runs_dev / its _u32 form / flashe_quantize_batch_encrypt_cohort_cut_runs_dev --
prf_chain_cohort_cut_kernel, prf_small_cohort_kernel and prf_chain_cohort_batch_cut_kernel<1024, 5 / 6 / 7> over the pieces of
cohort_cut_pieces, then cohort_cut_combine_kernel) against the present clients run one after the other as FlasheClient steps on one
quantiser state: every ciphertext, their sum, NumPy's generator, shape_dict, alpha_list, the floats of decrypt_unquantize and the mean /
std history, compared as bytes; the sum is also decrypted by the CPU oracle with the telescoped lists and held against the oracle's decrypt
of every ciphertext.  Outputs and scratch-sized blocks are poisoned first, `up.path` is asserted everywhere, and so is the piece count:
the planner's, the Python mirror's and the library's on the chip the test runs on.
tests/golden/clientstep.json records no round with dropped clients; its two batched int_bits > 64 cases run here through the batched cut."""
import functools
import hashlib
import operator

import numpy as np
import pytest

from conftest import load_golden, unhex
from test_gpu_cohort_cut import (COMPACT_WIDTHS, KEY, _arr, _expand, _ints, _models, _poison, _rng_states, _same_state, _TORCH_GPU,
                                 _values, _W)

pytestmark = pytest.mark.gpu


def _args(b, eb=16, batch=False):
    return {"quantize": {"int_bits": b, "batch": batch, "element_bits": eb, "padding": True, "secure": True}, "precompute": {"enable": False}}


def _sizes(n):
    """[1, 0, 300, rest]: a layer boundary inside the first pair of lanes' elements, an empty layer, a boundary mid-tile."""
    if n < 3:
        return [n]
    mid = min(300, n - 2)
    return [1, 0, mid, n - 1 - mid]


def _limbs(dv, compact):
    return _values(dv).reshape(-1, 1) if compact else np.asarray(dv.to_host(), dtype=np.uint64).reshape(-1, 2)


def _as_ints(limbs):
    limbs = np.asarray(limbs, dtype=np.uint64)
    return [int(r[0]) | ((int(r[1]) << 64) if limbs.shape[1] > 1 else 0) for r in limbs]


def _oracle_check(b, it, idxs, n_jobs, cts, psum, compact, mask):
    """The CPU oracle's decrypt of the sum with the telescoped lists is the sum of its decrypts of every ciphertext at that client's own
    index, and -- where the launch kept a mask -- the sum plus the mask."""
    from oracle import flashe_oracle as orc
    M = (1 << b) - 1
    add, minus = orc.telescope(list(idxs))
    runs = 1 + sum(1 for a, z in zip(idxs, idxs[1:]) if z != a + 1)
    assert len(add) == len(minus) == runs
    dec = _as_ints(orc.decrypt(KEY, it, add, minus, n_jobs, b, _limbs(psum, compact)))
    total = [0] * len(dec)
    for i, ct in zip(idxs, cts):
        pt = _as_ints(orc.decrypt(KEY, it, [i + 1], [i], n_jobs, b, _limbs(ct, compact)))
        total = [(t + p) & M for t, p in zip(total, pt)]
    assert dec == total, "the oracle's decrypt of the sum against its decrypts of the ciphertexts"
    if mask is not None:
        opened = [(s + m) & M for s, m in zip(_as_ints(_limbs(psum, False)), _as_ints(_limbs(mask, False)))]
        assert opened == dec, "sum + the kept mask against the oracle's decrypt with the telescoped lists"


def _round_trip(b, n, present=None, C=None, compact=False, eb=None, batch=False, sizes=None, normalize=False, rounds=1, first_idx=0, n_local=None,
                num_clients=None, want_path="cut-chain", prefer=None, cut="any", make_kw=dict, models_of=None, dtypes=("float32", "float64"),
                digest=None, n_jobs=16, want_runs=None):
    """`rounds` rounds of a cut="any" cohort against ONE FlasheClient whose cipher takes each present client's index in turn (one quantiser
    state, as the cohort has).  make_kw() builds the extra kwargs of the cohort call, once per side.  digest: every compared byte."""
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheClient, FlasheCohort, _telescoped, cohort_cut_items, cohort_cut_pieces
    cm.N_JOBS = n_jobs
    pos = list(range(C)) if present is None else list(present)
    C = len(pos)
    n_local = (max(pos) + 1) if n_local is None else n_local
    num_clients = n_local if num_clients is None else num_clients
    if eb is None:                                            # (the padded field fits int_bits: element_bits + ceil(log2 num_clients) <= b)
        eb = min(16, b - (num_clients - 1).bit_length())
    sizes = _sizes(n) if sizes is None else list(sizes)
    cl = FlasheClient(_args(b, eb, batch))
    cl.create_cipher(first_idx, num_clients, KEY)
    co = FlasheCohort(_args(b, eb, batch), first_idx=first_idx, n_local=n_local, num_clients=num_clients, prp_seed=KEY, compact=compact, cut=cut)
    co.prefer = prefer
    eng = co.cipher.engine
    elem = 4 if compact else 16
    idxs = [first_idx + p for p in pos]
    for it in range(rounds):
        models = (models_of or functools.partial(_models, dtypes=dtypes))(C, sizes, 100 + it)
        cl.set_iter_index(it)
        co.set_iter_index(it)
        np.random.seed(7 + it)
        np.random.random(3)                                   # an odd position in the stream
        state = np.random.get_state()
        kw_seq = make_kw()
        want = []
        for c in range(C):
            cl.cipher.idx = idxs[c]
            if kw_seq.get("seeds") is not None:
                np.random.seed(kw_seq["seeds"][c])
            w = cl.quantize_encrypt(_W(dict(models[c])), device=True, normalize=normalize, **_expand(kw_seq, c))
            want.append(w._weights[w.walking_order[0]])
        cl.cipher.idx = first_idx
        want_state = np.random.get_state()
        want_sum = cl.cipher.aggregate(want)
        plan = co.plan([_W(dict(m)) for m in models], None if present is None else pos)
        ne = plan.n_elems
        assert len(want_sum) == ne
        if want_runs is not None:
            assert plan.runs == want_runs
        if want_path == "cut-chain" and prefer is None:
            # the piece count: the planner's, the mirror's and the library's, on this chip
            mirror = cohort_cut_pieces(idxs, cohort_cut_items(plan.n, b, n_jobs, compact, ne if batch else None), eng.cu_count)
            assert plan.path == "cut-chain" and plan.parts == len(mirror) - 1 >= plan.runs, (plan.path, plan.reason, plan.parts, mirror)
            if hasattr(eng, "cohort_cut_pieces"):
                assert eng.cohort_cut_pieces(idxs, ne, n_jobs, compact=compact) == (plan.parts, mirror)
            if plan.runs > 1:
                assert plan.parts >= 2                        # a gapped cohort always runs the combine pass
        _poison(eng, [elem * ne] * (C + 2) + [max(plan.parts, 1) * ne * elem * (1 if compact else 2)])
        np.random.set_state(state)
        kw = make_kw()
        up = co.quantize_encrypt([_W(dict(m)) for m in models], normalize=normalize, **({} if present is None else {"present": pos}), **kw)
        assert up.path == want_path, (up.path, plan.path, plan.reason)
        assert up.present == idxs and len(up.ciphertexts) == C
        assert _same_state(np.random.get_state(), want_state), "the NumPy stream must be left where the sequential steps leave it"
        assert _rng_states(kw) == _rng_states(kw_seq), "the caller's generators must be left where the sequential steps leave them"
        for c in range(C):
            if compact:
                assert up.ciphertexts[c].elem_bytes == 4 and np.array_equal(_values(up.ciphertexts[c]), _values(want[c])), (it, c)
            else:
                assert up.ciphertexts[c].to_host().tobytes() == want[c].to_host().tobytes(), (it, c)
            if digest is not None:
                digest.update(_values(up.ciphertexts[c]).tobytes())
        if compact:
            assert np.array_equal(_values(up.partial_sum), _values(want_sum)), it
            assert co.lead._cohort_mask is None               # no mask is kept at the compact widths
        else:
            assert up.partial_sum.to_host().tobytes() == want_sum.to_host().tobytes(), it
        if digest is not None:
            digest.update(_values(up.partial_sum).tobytes())
        assert co.shape_dict == cl.shape_dict
        assert [float(a).hex() for a in co.quantizer.alpha_list] == [float(a).hex() for a in cl.quantizer.alpha_list]
        kept = co.lead._cohort_mask
        if C <= 48:
            _oracle_check(b, it, idxs, n_jobs, up.ciphertexts, up.partial_sum, compact, kept[1] if kept is not None else None)
        if num_clients != co.n_local:
            assert kept is None                               # clients outside the cohort: no mask is kept
            with pytest.raises(ValueError):
                co.decrypt_unquantize()
            continue
        assert (kept is not None) == (up.path in ("cut-chain", "cohort-chain") and not compact)
        if kept is not None:
            # the mask stands for the telescoped lists: decrypt_unquantize() is the one combine (+ unbatch) pass
            assert kept[0] == up.partial_sum.ptr and kept[2:] == (it,) + _telescoped(idxs) and len(kept[1]) == ne
        deg = {}
        if kw.get("degrees") is not None:
            deg = {"degree": kw["degrees"][0], "total_degree": functools.reduce(operator.add, kw["degrees"])}
        cl.set_idx_list(list(idxs))
        ref = cl.decrypt_unquantize(_W({sorted(models[0])[0]: want_sum}), unnormalize=True, **deg)
        got = co.decrypt_unquantize(unnormalize=True)
        assert got.walking_order == ref.walking_order
        for k in ref.walking_order:
            assert np.asarray(got._weights[k]).shape == np.asarray(ref._weights[k]).shape
            assert np.asarray(got._weights[k], dtype=np.float64).tobytes() == np.asarray(ref._weights[k], dtype=np.float64).tobytes(), (it, k)
            if digest is not None:
                digest.update(np.asarray(got._weights[k], dtype=np.float64).tobytes())
        qa, qb = co.quantizer, cl.quantizer
        assert [float(x).hex() for x in qa.past_layer_mean_list] == [float(x).hex() for x in qb.past_layer_mean_list]
        assert [float(x).hex() for x in qa.past_layer_std_list] == [float(x).hex() for x in qb.past_layer_std_list]
    return co


# ------------------------------------------------------------------------------------------------ wide, un-batched
# present, n_local: what the pattern exercises
PATTERNS = {
    "two-singles": ([0, 2], 3),                               # two one-client pieces
    "one-gap": ([0, 1, 3, 4], 5),
    "first-dropped": ([1, 2, 3, 4, 5], 6),                    # one run that does not start at the cohort's first cipher
    "last-dropped": ([0, 1, 2, 3, 4], 6),                     # one run, the decrypt told who uploaded
    "40-of-41": ([i for i in range(41) if i != 24], 41),      # runs of 24 and 16: the rule splits both
    "sixteen-runs": (list(range(0, 32, 2)), 32),              # every chain of the table a one-client piece
}


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("b", [65, 120, 128])
def test_wide_gapped_cut_cohort_is_the_present_clients_one_after_the_other(b, pattern):
    """One element, one short of a tile, one into the second tile, three tiles; layers [1, 0, 300, rest] in float32 / float64."""
    present, n_local = PATTERNS[pattern]
    for n in (1, 255, 257, 700):
        co = _round_trip(b, n, present=present, n_local=n_local)
        if pattern == "40-of-41" and co.cipher.engine.cu_count == 256:
            assert co.plan([_W(dict(m)) for m in _models(40, _sizes(n), 1)], present).parts == 10
        if pattern == "sixteen-runs":
            assert co.plan([_W(dict(m)) for m in _models(16, _sizes(n), 1)], present).parts == 16


def test_seventeen_runs_come_back_staged_with_the_same_bytes():
    co = _round_trip(128, 700, present=list(range(0, 34, 2)), want_path="staged-chain", want_runs=17)
    plan = co.plan([_W(dict(m)) for m in _models(17, _sizes(700), 1)], list(range(0, 34, 2)))
    assert plan.path == "staged-chain" and "17 runs" in plan.reason
    # and the library itself declines them, with nothing launched
    from flashe_amd import engine as E
    eng = E.Engine(KEY, 128, device=0)
    assert eng.cohort_cut_pieces(list(range(0, 34, 2)), 700, 16) == (0, [])
    assert eng.cohort_cut_pieces(list(range(0, 32, 2)), 700, 16) == (16, list(range(17)))
    for bad in ([3, 2], [2, 2], [1, 2 ** 32 - 1]):
        with pytest.raises(E.FlasheError) as ei:
            eng.cohort_cut_pieces(bad, 700, 16)
        assert ei.value.code == -22


def test_a_gapped_cut_cohort_inside_a_larger_federation_keeps_no_mask():
    _round_trip(128, 700, present=[0, 1, 4, 5], first_idx=3, n_local=6, num_clients=12)
    _round_trip(20, 700, present=[0, 1, 4, 5], first_idx=3, n_local=6, num_clients=12, compact=True)


def test_two_normalised_rounds_with_a_gap():
    """The statistics the first round's decrypt leaves feed the second round's alphas and shifts."""
    _round_trip(128, 700, present=[0, 1, 3, 4], normalize=True, rounds=2)
    _round_trip(120, 700, present=[0, 2, 3, 4], normalize=True, rounds=2, batch=True, sizes=(7, 300, 1, 393))


@pytest.mark.parametrize("dtype", ["float64", "float16"])
def test_a_model_of_one_dtype_with_a_gap(dtype):
    _round_trip(128, 700, present=[0, 1, 3, 4], dtypes=(dtype,))
    _round_trip(128, 700, present=[0, 1, 3, 4], dtypes=(dtype,), batch=True, sizes=(7, 300, 1, 393))


def test_float16_tensors_with_a_gap():
    torch = pytest.importorskip("torch")
    if not (_TORCH_GPU and torch.cuda.is_available()):
        pytest.skip("no GPU visible to torch")

    def tensors(C, sizes, seed):
        return [{k: torch.from_numpy(np.asarray(v, dtype=np.float32)).to("cuda").to(torch.float16) for k, v in m.items()}
                for m in _models(C, sizes, seed, dtypes=("float32",))]
    _round_trip(128, 700, present=[0, 1, 3, 4], normalize=True, models_of=tensors, sizes=[1, 300, 399])
    _round_trip(128, 700, present=[0, 1, 3, 4], models_of=tensors, sizes=[1, 300, 399], batch=True)


def test_degrees_and_one_philox_generator_with_a_gap():
    _round_trip(128, 700, present=[0, 1, 3, 4], normalize=True, make_kw=lambda: {"degrees": [3, 5, 2, 7]})
    _round_trip(128, 700, present=[0, 1, 3, 4], make_kw=lambda: {"rng": np.random.Generator(np.random.Philox(key=40))})
    _round_trip(128, 700, batch=True, C=5, sizes=(7, 300, 1, 393), make_kw=lambda: {"rng": np.random.Generator(np.random.Philox(key=41))})


# ------------------------------------------------------------------------------------------------ compact
TWENTY_OF_23 = [i for i in range(23) if i not in (4, 11, 12)]


@pytest.mark.parametrize("n_jobs", [1, 16])
@pytest.mark.parametrize("b,eb", COMPACT_WIDTHS)
def test_compact_gapped_cut_cohort_at_every_width(b, eb, n_jobs):
    """n = 5 (fewer elements than chunks at N_JOBS 16: every block partial), 700, and 4,099 (a partial last block in some chunks and more than
    one tile at every width); the decrypt goes through the telescoped lists."""
    for n in (5, 700, 4099):
        _round_trip(b, n, present=[0, 1, 3, 4], compact=True, eb=eb, n_jobs=n_jobs)
    _round_trip(b, 700, present=TWENTY_OF_23, compact=True, eb=min(eb, b - 5), n_jobs=n_jobs, normalize=True)


# ------------------------------------------------------------------------------------------------ batched
# sizes that are no multiples of bs, a layer boundary inside a half tile, a layer shorter than one element: 1, ~130 .. 180 and ~300 .. 420 elements
BATCH_SIZES = {"one-element": (3,), "two-half-tiles": (7, 300, 1, 600), "two-tiles": (7, 300, 1, 1800)}
BATCH_SHAPES = [(120, 10, 6), (128, 3, 7), (128, 10, 6), (128, 100, 5)]        # int_bits, num_clients -> bs at element_bits 16


def _batch_patterns(num_clients):
    if num_clients == 3:
        return [None, [0, 2]]
    mid = num_clients // 2
    return [None, [i for i in range(num_clients) if i != mid], [i for i in range(num_clients) if i not in (1, mid, mid + 1)]]


@pytest.mark.parametrize("shape", list(BATCH_SIZES))
@pytest.mark.parametrize("b,num_clients,bs", BATCH_SHAPES)
def test_batched_cut_cohort_is_the_present_clients_one_after_the_other(b, num_clients, bs, shape):
    from flashe_amd.block import _field_bits
    assert b // _field_bits(16, num_clients) == bs
    sizes = BATCH_SIZES[shape]
    for runs, present in enumerate(_batch_patterns(num_clients), 1):
        co = _round_trip(b, sum(sizes), present=present, C=num_clients, n_local=num_clients, batch=True, sizes=sizes, eb=16, want_runs=runs)
        assert co.lead._cohort_mask is not None and len(co._last.partial_sum) == sum(-(-s // bs) for s in sizes)


_DENSE = load_golden("clientstep.json")["dense"]
_RECORDED_BATCHED = [i for i, c in enumerate(_DENSE) if c["scheme"] == "double" and c.get("batch") and c["b"] > 64]


@pytest.mark.parametrize("case_i", _RECORDED_BATCHED)
def test_batched_cut_cohort_is_the_reference_jobs_client_steps(case_i):
    """The batched double-mask cases of tests/golden/clientstep.json at int_bits 128 (ten clients, bs 6) and 120 (three clients, bs 7),
    recorded by calling the reference with per-client seeds, through a cut="any" cohort."""
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheCohort
    case = _DENSE[case_i]
    assert len(_RECORDED_BATCHED) == 2
    b, C = case["b"], case["num_clients"]
    cm.N_JOBS = case["n_jobs"]
    co = FlasheCohort(_args(b, case["element_bits"], True), first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, cut="any")
    co.set_iter_index(case["iter"])
    ws = [_W({nm: _arr(rec["layers"][nm], np.dtype(dt), sh) for nm, sh, dt in case["layers"]}) for rec in case["clients"]]
    _poison(co.cipher.engine, [16 * case["n"]] * (C + 4))
    up = co.quantize_encrypt(ws, seeds=[rec["seed"] for rec in case["clients"]])
    assert up.path == "cut-chain" and len(up.ciphertexts) == C
    for c, rec in enumerate(case["clients"]):
        assert [int(v) for v in _ints(up.ciphertexts[c], False)] == unhex(rec["flat_ct"]), (b, c)
        assert [float(a).hex() for a in co.quantizer.alpha_list] == rec["alpha"]
        assert {k: list(sh) for k, sh in co.shape_dict.items()} == rec["shape_dict"]
    assert [int(v) for v in _ints(up.partial_sum, False)] == unhex(case["agg_elem"])
    assert co.lead._cohort_mask is not None
    back = co.decrypt_unquantize()
    for nm, sh, _dt in case["layers"]:
        a = back._weights[nm]
        assert a.shape == tuple(sh)
        assert np.asarray(a, dtype=np.float64).tobytes() == bytes.fromhex(case["out_elem"]["unquantized"][nm]), (b, nm)


# ------------------------------------------------------------------------------------------------ equivalences
def test_one_run_unbatched_is_the_cut_true_launch():
    for kw in ({"b": 128}, {"b": 20, "compact": True}):
        a, t = hashlib.sha256(), hashlib.sha256()
        _round_trip(kw["b"], 700, C=17, compact=kw.get("compact", False), digest=a)
        _round_trip(kw["b"], 700, C=17, compact=kw.get("compact", False), cut=True, digest=t)
        assert a.digest() == t.digest()


@pytest.mark.parametrize("kw", [{"b": 128, "present": [0, 1, 3, 4]}, {"b": 128, "present": PATTERNS["40-of-41"][0]},
                                {"b": 23, "present": TWENTY_OF_23, "compact": True},
                                {"b": 128, "present": [0, 2, 3, 4], "batch": True, "sizes": (7, 300, 1, 600)},
                                {"b": 120, "C": 10, "batch": True, "sizes": (7, 300, 1, 600)}],
                         ids=["gap", "40-of-41", "compact-20-of-23", "batched-gap", "batched"])
def test_prefer_staged_gives_the_same_bytes(kw):
    kw = dict(kw)
    b = kw.pop("b")
    n = sum(kw["sizes"]) if "sizes" in kw else 700
    a, s = hashlib.sha256(), hashlib.sha256()
    _round_trip(b, n, digest=a, **kw)
    _round_trip(b, n, digest=s, prefer="staged-chain", want_path="staged-chain", **kw)
    assert a.digest() == s.digest()


def test_cut_true_still_runs_these_shapes_staged():
    _round_trip(128, 700, present=[0, 1, 3, 4], cut=True, want_path="staged-chain")
    _round_trip(128, 700, C=5, batch=True, sizes=(7, 300, 1, 393), cut=True, want_path="staged-chain")


# ------------------------------------------------------------------------------------------------ the raw entry points
def _raw(eng, idx, n, compact):
    from flashe_amd import _lib
    C, elem = len(idx), 4 if compact else 16
    x, u = eng.upload(np.linspace(-0.4, 0.4, n).astype(np.float32)), eng.upload(np.random.Generator(np.random.PCG64(1)).random(C * n))
    rows, srcs, dts = [(0, None, 0.5, 0.0, _lib.TENSOR_F32, 0)], [[x.ptr]] * C, [[_lib.TENSOR_F32]] * C
    cts, dsum, dmask = [eng.alloc(elem * n) for _ in range(C)], eng.alloc(elem * n), eng.alloc(elem * n)
    for d in cts + [dsum, dmask]:
        eng.memset_dev(d, 0xA5, elem * n)
    return (3, idx, n, 16, rows, srcs, dts, 16, u, cts, dsum), dmask, (x, u)


def _untouched(eng, bufs, n, elem):
    eng.sync()
    return all((d.download(np.uint8, elem * n) == 0xA5).all() for d in bufs)


def test_the_raw_entry_points_refuse_bad_arguments_and_decline_untouched():
    from flashe_amd import engine as E
    n, idx = 700, [0, 1, 3, 4]
    for compact, b in ((False, 128), (True, 20)):
        eng = E.Engine(KEY, b, device=0)
        elem = 4 if compact else 16
        parts, begins = eng.cohort_cut_pieces(idx, n, 16, compact=compact)
        assert (parts, begins) == (2, [0, 2, 4])
        a, dmask, _keep = _raw(eng, idx, n, compact)
        call = eng.quantize_encrypt_cohort_cut_runs_u32_dev if compact else functools.partial(eng.quantize_encrypt_cohort_cut_runs_dev, dmask=dmask)
        scratch = eng.alloc(2 * parts * n * elem + 64)
        for bad in (None, E.DeviceBufferView(scratch, 8, parts * n * elem), a[9][0], a[10]) + (() if compact else (dmask,)):
            with pytest.raises(E.FlasheError) as ei:
                call(*a, scratch=bad)
            assert ei.value.code == -22
        for bad_idx in ([0, 1, 1, 4], [0, 3, 1, 4], [0, 1, 3, 2 ** 32 - 1]):
            with pytest.raises(E.FlasheError) as ei:
                call(*(a[:1] + (bad_idx,) + a[2:]), scratch=scratch)
            assert ei.value.code == -22
        assert _untouched(eng, a[9] + [a[10], dmask], n, elem)
        assert call(*a, scratch=scratch) is True
        eng.sync()
        assert not (a[10].download(np.uint8, elem * n) == 0xA5).all()
    # seventeen runs and int_bits 64: declined, nothing launched
    eng = E.Engine(KEY, 128, device=0)
    idx = list(range(0, 34, 2))
    a, dmask, _keep = _raw(eng, idx, n, False)
    assert eng.quantize_encrypt_cohort_cut_runs_dev(*a, dmask=dmask, scratch=eng.alloc(2 * 16 * n * 16)) is False
    assert _untouched(eng, a[9] + [a[10], dmask], n, 16)
    e64 = E.Engine(KEY, 64, device=0)
    a, dmask, _keep = _raw(e64, [0, 1, 3, 4], n, False)
    assert e64.cohort_cut_pieces([0, 1, 3, 4], n, 16) == (0, [])
    assert e64.quantize_encrypt_cohort_cut_runs_dev(*a, scratch=e64.alloc(4096)) is False
    assert _untouched(e64, a[9] + [a[10]], n, 16)
