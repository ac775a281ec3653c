"""CPU test: the rng= argument of the layers that draw -- _static_quantize_padding_asymmetric, QuantizingClient.quantize,
FlasheClient.quantize_encrypt, FlasheCohort.quantize_encrypt (on the recording engine double of tests/test_cohort_batch_planner.py) and
FlasheSparseCohort.quantize_encrypt (on the computing double of tests/test_sparse_cohort_front_end_planner.py).  Every refusal leaves the
quantiser, the generators, NumPy's global state and the cohort's last upload untouched; rng=None issues the calls it always issued; a list
of C Philox generators is ONE philox_random_dev call of C segments at offsets c * per_client; a PCG64 generator takes the upload path and
is advanced by exactly the draws consumed; and the sparse cohort's result with rng=G is that of the same call with np.random.random
replaced by G.random.  Touches no device and no library."""
import numpy as np
import pytest

from test_cohort_batch_planner import KEY, RecordingEngine, _args, _Buf, _W
from test_sparse_cohort_front_end_planner import SparseEngine
from test_sparse_cohort_front_end_planner import _args as _sparse_args

SIZES = [7, 0, 70001]                       # per client: 70,008 values, above DEVICE_RNG_MIN
N = sum(SIZES)
LAUNCHES = ["quantize_batch_tensors_dev"] * 3 + ["encrypt_batch_sum_dev"]         # the staged form: what this shape runs on two CUs


class _RecBuf(_Buf):
    def upload_at(self, off, arr):
        super().upload_at(off, arr)
        if np.asarray(arr).dtype == np.float64:                  # draws (the layers of these tests are float32)
            self.engine.log.append(("upload_at", off, int(np.asarray(arr).size)))
        return self


class RngEngine(RecordingEngine):
    """RecordingEngine + the draw calls, recorded; the generators are advanced as the device calls advance them."""
    PHILOX_MAX_SEGMENTS = 128

    def alloc(self, nbytes):
        return _RecBuf(self, nbytes)

    def numpy_random_dev(self, n, out=None):
        self._rec("numpy_random_dev", n, out)
        np.random.random(n)
        return out

    def philox_random_dev(self, generators, counts, out=None, offsets=None):
        self._rec("philox_random_dev", list(generators), list(counts), out, list(offsets))
        for g, n in zip(generators, counts):
            g.random(n)
        return out


def _philox(seed):
    return np.random.Generator(np.random.Philox(key=seed))


def _cohort(monkeypatch, n_local=3):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheCohort
    monkeypatch.setattr(cm.FlasheCipher, "_engine_cls", RngEngine)
    monkeypatch.setattr(cm, "N_JOBS", 16)
    co = FlasheCohort(_args(120), first_idx=0, n_local=n_local, num_clients=n_local, prp_seed=KEY)
    co.set_iter_index(4)
    ws = [_W({f"l{i}": np.zeros(s, np.float32) for i, s in enumerate(SIZES)}) for _ in range(n_local)]
    return co, ws


def _state_bytes(g):
    st = g.bit_generator.state
    return repr(sorted((k, v.tobytes() if isinstance(v, np.ndarray) else repr(v)) for k, v in
                       list(st.items()) + list(st["state"].items()) if not isinstance(v, dict)))


def _global_bytes():
    st = np.random.get_state()
    return st[1].tobytes(), st[2]


def _draw_calls(log):
    return [e for e in log if e in ("numpy_random_dev", "philox_random_dev") or isinstance(e, tuple)]


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_of_the_cohort_leaves_everything_untouched(monkeypatch):
    co, ws = _cohort(monkeypatch)
    q, eng = co.lead.quantizer, co.cipher.engine
    gens = [_philox(s) for s in (1, 2, 3)]
    np.random.seed(5)
    co._last, co.lead._cohort_mask = "last", "mask"
    before = (_global_bytes(), [_state_bytes(g) for g in gens], q.alpha_list, q.r_max_list, q.layer_size_list)
    cases = [(dict(rng=gens, seeds=[1, 2, 3]), ValueError), (dict(rng=gens[0], seeds=[1, 2, 3]), ValueError),
             (dict(rng=gens[:2]), ValueError), (dict(rng=gens + gens[:1]), ValueError),
             (dict(rng="philox"), TypeError), (dict(rng=7), TypeError), (dict(rng=np.random.RandomState(1)), TypeError),
             (dict(rng=np.random.Philox(1)), TypeError), (dict(rng=[gens[0], 3, gens[2]]), TypeError),
             (dict(rng=gens[:2], present=[0, 2], seeds=[1, 2]), ValueError), (dict(rng=gens, present=[0, 2]), ValueError)]
    for kw, err in cases:
        with pytest.raises(err):
            co.quantize_encrypt(ws[:2] if "present" in kw else ws, **kw)
        after = (_global_bytes(), [_state_bytes(g) for g in gens], q.alpha_list, q.r_max_list, q.layer_size_list)
        assert after == before and eng.log == [] and co._last == "last" and co.lead._cohort_mask == "mask", kw


def test_the_other_layers_refuse_before_they_touch_anything():
    from flashe_amd.block import FlasheClient
    from flashe_amd.quantize import QuantizingClient, _static_quantize_padding_asymmetric
    np.random.seed(6)
    before = _global_bytes()
    g = _philox(4)
    gb = _state_bytes(g)
    with pytest.raises(ValueError):
        _static_quantize_padding_asymmetric(np.zeros(4), 1.0, 16, uniforms=np.zeros(4), rng=g)
    with pytest.raises(TypeError):
        _static_quantize_padding_asymmetric(np.zeros(4), 1.0, 16, rng="g")
    qc = QuantizingClient(64, element_bits=16)
    qc.num_clients, qc.layer_size_list = 2, [4]
    w = _W({"a": np.zeros(4)})
    for bad in ([g], np.random.default_rng, 0.5):
        with pytest.raises(TypeError):
            qc.quantize(w, rng=bad)
        assert qc.alpha_list is None and qc.r_max_list is None and w._weights["a"].dtype == np.float64
    cl = FlasheClient(_args(64))
    for bad in ([g], "g"):
        with pytest.raises(TypeError):
            cl.quantize_encrypt(w, rng=bad)
        with pytest.raises(TypeError):
            cl.quantize(w, rng=bad)
    assert _global_bytes() == before and _state_bytes(g) == gb and list(w._weights) == ["a"]


# ------------------------------------------------------------------------------------------------------------------ the cohort's draw calls
def test_rng_none_issues_the_calls_it_always_issued(monkeypatch):
    # host draws: the global stream is read in one stretch of C n draws and uploaded, nothing else is asked of the engine
    monkeypatch.setenv("FLASHE_DEVICE_RNG", "0")
    co, ws = _cohort(monkeypatch)
    np.random.seed(3)
    up = co.quantize_encrypt(ws)
    assert up.path == "staged-chain" and co.cipher.engine.log == [("upload_at", 0, 3 * N)] + LAUNCHES
    after = _global_bytes()
    np.random.seed(3)
    np.random.random(3 * N)
    assert _global_bytes() == after
    # device draws: the MT19937 call, never the Philox one
    monkeypatch.setenv("FLASHE_DEVICE_RNG", "1")
    co, ws = _cohort(monkeypatch)
    np.random.seed(3)
    co.quantize_encrypt(ws, rng=None)
    eng = co.cipher.engine
    assert eng.log == ["numpy_random_dev"] + LAUNCHES and eng.args["numpy_random_dev"][0] == 3 * N
    assert _global_bytes() == after
    # seeds: one stretch per client
    co, ws = _cohort(monkeypatch)
    co.quantize_encrypt(ws, seeds=[5, 6, 7])
    assert co.cipher.engine.log == ["numpy_random_dev"] * 3 + LAUNCHES


def test_a_list_of_philox_generators_is_one_launch_of_c_segments(monkeypatch):
    monkeypatch.delenv("FLASHE_DEVICE_RNG", raising=False)
    co, ws = _cohort(monkeypatch)
    gens = [_philox(s) for s in (1, 2, 3)]
    np.random.seed(9)
    before = _global_bytes()
    up = co.quantize_encrypt(ws, rng=gens)
    eng = co.cipher.engine
    assert up.path == "staged-chain" and eng.log == ["philox_random_dev"] + LAUNCHES
    g, counts, out, offsets = eng.args["philox_random_dev"]
    assert all(a is b for a, b in zip(g, gens)) and counts == [N] * 3 and offsets == [0, N, 2 * N] and out.nbytes == 8 * 3 * N
    assert eng.args["quantize_batch_tensors_dev"][4] == out.ptr + 8 * 2 * N               # the last client's launch reads its segment
    assert _global_bytes() == before
    # one Generator for the whole cohort: one segment of C n draws
    co, ws = _cohort(monkeypatch)
    one = _philox(8)
    co.quantize_encrypt(ws, rng=one)
    eng = co.cipher.engine
    assert _draw_calls(eng.log) == ["philox_random_dev"] and eng.args["philox_random_dev"][1:] == ([3 * N], eng.args["philox_random_dev"][2], [0])
    # dropped-out clients: one generator per PRESENT client
    co, ws = _cohort(monkeypatch)
    co.quantize_encrypt(ws[:2], rng=gens[:2], present=[0, 2])
    assert _draw_calls(co.cipher.engine.log) == ["philox_random_dev"] and co.cipher.engine.args["philox_random_dev"][3] == [0, N]
    # FLASHE_DEVICE_RNG=0: the same generators draw on the host
    monkeypatch.setenv("FLASHE_DEVICE_RNG", "0")
    co, ws = _cohort(monkeypatch)
    co.quantize_encrypt(ws, rng=gens)
    assert _draw_calls(co.cipher.engine.log) == [("upload_at", 8 * c * N, N) for c in range(3)]


def test_a_pcg64_generator_uploads_and_advances_by_the_draws_consumed(monkeypatch):
    monkeypatch.delenv("FLASHE_DEVICE_RNG", raising=False)
    co, ws = _cohort(monkeypatch)
    g, twin = np.random.Generator(np.random.PCG64(21)), np.random.Generator(np.random.PCG64(21))
    np.random.seed(9)
    before = _global_bytes()
    co.quantize_encrypt(ws, rng=g)
    assert _draw_calls(co.cipher.engine.log) == [("upload_at", 0, 3 * N)]
    twin.random(3 * N)
    assert _state_bytes(g) == _state_bytes(twin) and _global_bytes() == before
    # a list: client c's stretch from rng[c], each advanced by n
    co, ws = _cohort(monkeypatch)
    gens = [np.random.Generator(np.random.PCG64(s)) for s in (1, 2, 3)]
    twins = [np.random.Generator(np.random.PCG64(s)) for s in (1, 2, 3)]
    co.quantize_encrypt(ws, rng=gens)
    assert _draw_calls(co.cipher.engine.log) == [("upload_at", 8 * c * N, N) for c in range(3)]
    for t in twins:
        t.random(N)
    assert [_state_bytes(x) for x in gens] == [_state_bytes(t) for t in twins]
    # mixed: the Philox clients in one launch, the PCG64 client on the host
    co, ws = _cohort(monkeypatch)
    mixed = [_philox(1), np.random.Generator(np.random.PCG64(2)), _philox(3)]
    co.quantize_encrypt(ws, rng=mixed)
    eng = co.cipher.engine
    assert _draw_calls(eng.log) == [("upload_at", 8 * N, N), "philox_random_dev"] and eng.args["philox_random_dev"][3] == [0, 2 * N]


# ------------------------------------------------------------------------------------------------------------------ the sparse cohort, computed
def _sparse_round(monkeypatch, rng=None, patch=None, seeds=None):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheSparseCohort
    monkeypatch.setattr(cm.FlasheCipher, "_engine_cls", SparseEngine)
    monkeypatch.setattr(cm, "N_JOBS", 4)
    ks, total, C = (4, 1, 30), 400, 3
    g = np.random.Generator(np.random.PCG64(11))
    co = FlasheSparseCohort(_sparse_args(20), first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, sparsity=0.1)
    co.set_iter_index(2)
    masks = [np.sort(g.choice(total, sum(ks), replace=False)) for _ in range(C)]
    assert co.dynamic_masking("single", [m.tolist() for m in masks], total) == "single"
    compact = [{f"l{i}": (g.standard_normal(k) * 0.05).astype(np.float64 if i == 1 else np.float32) for i, k in enumerate(ks)} for _ in range(C)]
    if patch is not None:
        monkeypatch.setattr(np.random, "random", patch)
    try:
        up = co.quantize_encrypt(compact=compact, normalize=True, rng=rng, seeds=seeds)
    finally:
        monkeypatch.undo()
    return ([u.to_host().tobytes() for u in up.uploads], up.aggregate.to_host().tobytes(), [float(a).hex() for a in co.alpha_list], dict(co.shape_dict))


@pytest.mark.parametrize("bitgen", [np.random.Philox, np.random.PCG64])
def test_the_sparse_cohort_with_rng_is_the_call_with_np_random_random_replaced(monkeypatch, bitgen):
    np.random.seed(12)
    before = _global_bytes()
    ref_g, g = np.random.Generator(bitgen(5)), np.random.Generator(bitgen(5))
    ref = _sparse_round(monkeypatch, patch=ref_g.random)
    got = _sparse_round(monkeypatch, rng=g)
    assert got == ref and _state_bytes(g) == _state_bytes(ref_g) and _global_bytes() == before
    # a list: client c draws its K + 1 values from rng[c]
    gens = [np.random.Generator(bitgen(s)) for s in (1, 2, 3)]
    twins = [np.random.Generator(bitgen(s)) for s in (1, 2, 3)]
    got = _sparse_round(monkeypatch, rng=gens)
    for t in twins:
        t.random(36)
    assert [_state_bytes(x) for x in gens] == [_state_bytes(t) for t in twins] and _global_bytes() == before
    assert got[2:] == ref[2:] and got[0] != ref[0]
    with pytest.raises(ValueError):
        _sparse_round(monkeypatch, rng=gens, seeds=[1, 2, 3])
    with pytest.raises(ValueError):
        _sparse_round(monkeypatch, rng=gens[:2])
    with pytest.raises(TypeError):
        _sparse_round(monkeypatch, rng=[gens[0], "g", gens[2]])
    assert [_state_bytes(x) for x in gens] == [_state_bytes(t) for t in twins] and _global_bytes() == before
