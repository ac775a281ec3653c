"""CPU test: the degree / total_degree / last_round arguments of FlasheClient, FlasheCohort and FlasheSparseCohort on host layers.

The cipher runs on the oracle-backed engine double of tests/fake_engine.py and the quantiser's codec on a NumPy double built from
tests/codec_ref.py (the formulas the codec kernels are pinned to), so the call-by-call step computes real numbers without a device.  The
yardstick is the reference's own sequence written out with NumPy (jzf_aggregator.py:676, :902-907): `layer * degree` before the existing
quantize_encrypt(normalize=True); the existing decrypt_unquantize, `/ (total / degree)`, the existing unnormalize, `/ degree` and
`last + w` after it, with the same np.random.seed.  Bytes and hex forms are compared; there is no tolerance."""
import functools
import operator

import numpy as np
import pytest

import codec_ref
from fake_engine import OracleEngine
from test_cohort_batch_planner import RecordingEngine
from trace_client_step import FakeTensor

KEY = bytes(range(32))
DEGREES = [5000.0, 3, np.float64(37.0), np.float32(0.3)]
IDS = ["float", "int", "np.float64", "np.float32"]


class _W:
    def __init__(self, layers):
        self.walking_order = sorted(layers)
        self._weights = dict(layers)


class _HostBuf:
    def __init__(self, arr):
        self.arr = arr

    def download(self, dtype, count):
        assert self.arr.dtype == dtype and self.arr.size == count
        return self.arr.copy()


class CodecEngine:
    """The quantiser's codec engine in NumPy: quantize / unquantize by tests/codec_ref.py, shift_dev as NumPy's in-place add."""

    def __init__(self, key, int_bits, device=0, stream=None):
        self.int_bits, self.limbs = int_bits, 2 if int_bits > 64 else 1

    def upload(self, arr):
        return _HostBuf(np.array(arr, copy=True))

    def shift_dev(self, n, d, is_f64, shift, wide):
        assert d.arr.size == n and (d.arr.dtype == np.float64) == bool(is_f64)
        d.arr += np.float64(shift) if wide or is_f64 else float(shift)

    def quantize(self, x, alpha, element_bits, u):
        return codec_ref.ref_quantize(x, alpha, element_bits, u).astype(np.uint64)

    def unquantize(self, v, alpha, element_bits, num_clients):
        v = np.asarray(v)
        ints = [int(a) | (int(b) << 64) for a, b in v] if v.ndim == 2 else [int(a) for a in v]
        return codec_ref.ref_unquantize(ints, alpha, element_bits, num_clients)


@pytest.fixture()
def doubles(oracle, monkeypatch):
    from flashe_amd import cipher as cm, quantize as qm
    monkeypatch.setattr(cm.FlasheCipher, "_engine_cls", OracleEngine)
    monkeypatch.setattr(qm, "Engine", CodecEngine)
    monkeypatch.setattr(qm, "_engines", {})
    monkeypatch.setattr(cm, "N_JOBS", 4)
    monkeypatch.setenv("FLASHE_DEVICE_RNG", "0")


def _args(b, batch=False):
    return {"quantize": {"int_bits": b, "batch": batch, "element_bits": 16, "padding": True, "secure": True}, "precompute": {"enable": False}}


def _client(b=64, scale=1.0):
    """A keyed client with the statistics a previous round leaves (np.float64 means and stds of a model scaled by `scale`)."""
    from flashe_amd.block import FlasheClient
    cl = FlasheClient(_args(b))
    cl.create_cipher(0, 3, KEY)
    cl.set_iter_index(2)
    q = cl.quantizer
    q.layer_size_list = [129, 129, 33]
    q.past_layer_mean_list = [np.float64(0.0123 * scale * (i + 1)) for i in range(3)]
    q.past_layer_std_list = [np.float64(0.05 * scale) for _ in range(3)]
    return cl


def _layers(seed=1):
    g = np.random.Generator(np.random.PCG64(seed))
    return {"a": (g.standard_normal(129) * 0.05).astype(np.float32), "b": (g.standard_normal((3, 43)) * 0.05).astype(np.float32),
            "c": g.standard_normal(33) * 0.05}


def _hex(xs):
    return [float(x).hex() for x in xs]


def _state(cl):
    q = cl.quantizer
    st = np.random.get_state()
    return (_hex(q.past_layer_mean_list), _hex(q.past_layer_std_list), q.alpha_list, q.r_max_list, list(q.layer_size_list), cl.shape_dict,
            st[1].tobytes(), st[2])


def _ct(w):
    v = w._weights[w.walking_order[0]]
    return [int(x) for x in np.asarray(v).reshape(-1)]


# ------------------------------------------------------------------------------------------------------------------ the front
@pytest.mark.parametrize("degree", DEGREES, ids=IDS)
@pytest.mark.parametrize("b", [64, 128])
def test_quantize_encrypt_with_a_degree_is_the_premultiplied_call(doubles, b, degree):
    layers = _layers()
    before = {k: v.copy() for k, v in layers.items()}
    ref, got = _client(b, float(degree)), _client(b, float(degree))
    np.random.seed(7)
    want = ref.quantize_encrypt(_W({k: v * degree for k, v in layers.items()}), device=False, normalize=True)
    np.random.seed(7)
    mine = _W(dict(layers))
    res = got.quantize_encrypt(mine, device=False, normalize=True, degree=degree)
    assert _ct(res) == _ct(want) and len(_ct(res)) == 129 + 129 + 33
    assert _state(got) == _state(ref) and got.degree is degree and ref.degree is None
    for k in layers:                                              # the caller's arrays: the same objects, the same bytes
        assert layers[k].tobytes() == before[k].tobytes() and layers[k].dtype == before[k].dtype
    # the dtype rule is NumPy's own: a Python number is weak, an np.float64 widens a float32 layer
    assert (layers["a"] * degree).dtype == (np.float64 if isinstance(degree, np.float64) else np.float32)


def test_the_sparse_jobs_zzz_value_is_not_scaled(doubles):
    layers = dict(_layers(), zzz=np.array([0.25], dtype=np.float32))
    ref, got = _client(), _client()
    for cl in (ref, got):
        cl.quantizer.layer_size_list, cl.quantizer.past_layer_mean_list, cl.quantizer.past_layer_std_list = None, [], []
    np.random.seed(3)
    want = ref.quantize_encrypt(_W({k: (v if k == "zzz" else v * 5000.0) for k, v in layers.items()}), device=False)
    np.random.seed(3)
    res = got.quantize_encrypt(_W(dict(layers)), device=False, degree=5000.0)
    assert _ct(res) == _ct(want) and len(_ct(res)) == 129 + 129 + 33 + 1


# ------------------------------------------------------------------------------------------------------------------ the back
def _round(degree):
    """(ref, got, aggregate): two clients in the state behind the same quantize_encrypt, and its upload as the aggregate."""
    ref, got = _client(64, float(degree)), _client(64, float(degree))
    ups = []
    for cl in (ref, got):
        np.random.seed(7)
        ups.append(cl.quantize_encrypt(_W(dict(_layers())), device=False, normalize=True, degree=degree))
        cl.set_idx_list([0, 1, 2])
    return ref, got, np.asarray(ups[0]._weights["a"])


@pytest.mark.parametrize("degree, total", [(5000.0, 13700), (np.float64(37.0), 111), (3, 10), (np.float32(0.3), 1.5)], ids=IDS)
@pytest.mark.parametrize("with_last", [False, True])
@pytest.mark.parametrize("unnormalize", [False, True])
def test_decrypt_unquantize_with_degrees_is_the_written_out_sequence(doubles, degree, total, with_last, unnormalize):
    ref, got, agg = _round(degree)
    last = {k: (v * 3).astype(np.float32) for k, v in _layers(5).items()} if with_last else None
    w = ref.decrypt_unquantize(_W({"a": agg.copy()}))
    for k in w.walking_order:
        w._weights[k] = w._weights[k] / (total / degree)
    if unnormalize:
        w = ref.unnormalize(w)
    for k in w.walking_order:
        w._weights[k] = w._weights[k] / degree
        if with_last:
            w._weights[k] = last[k] + w._weights[k]
    res = got.decrypt_unquantize(_W({"a": agg.copy()}), unnormalize=unnormalize, total_degree=total, last_round=_W(last) if with_last else None)
    assert res.walking_order == w.walking_order == ["a", "b", "c"]
    for k in w.walking_order:
        assert res._weights[k].dtype == w._weights[k].dtype == np.float64 and res._weights[k].shape == w._weights[k].shape
        assert res._weights[k].tobytes() == w._weights[k].tobytes(), k
    assert _hex(got.quantizer.past_layer_mean_list) == _hex(ref.quantizer.past_layer_mean_list)
    assert _hex(got.quantizer.past_layer_std_list) == _hex(ref.quantizer.past_layer_std_list)
    # an explicit degree, and last_round as a plain dict, give the same
    _r2, g2, _agg = _round(degree)
    g2.degree = None
    again = g2.decrypt_unquantize(_W({"a": agg.copy()}), unnormalize=unnormalize, degree=degree, total_degree=total, last_round=last)
    assert all(again._weights[k].tobytes() == w._weights[k].tobytes() for k in w.walking_order)


def test_without_degrees_nothing_changes(doubles):
    ref, got, agg = _round(5000.0)
    a = ref.unnormalize(ref.decrypt_unquantize(_W({"a": agg.copy()})))
    b = got.decrypt_unquantize(_W({"a": agg.copy()}), unnormalize=True)          # the remembered degree alone scales nothing
    assert all(a._weights[k].tobytes() == b._weights[k].tobytes() for k in a.walking_order)
    assert _hex(got.quantizer.past_layer_mean_list) == _hex(ref.quantizer.past_layer_mean_list)


# ------------------------------------------------------------------------------------------------------------------ refusals
BAD = [0, 0.0, -1.0, float("inf"), float("nan"), "5", 1j, [5.0], True, np.float64(0.0), np.array(5.0)]


def test_every_refusal_leaves_the_quantiser_and_the_stream_untouched(doubles):
    cl = _client()
    np.random.seed(11)
    layers = _layers()
    before = _state(cl)
    for bad in BAD:
        w = _W(dict(layers))
        with pytest.raises(ValueError):
            cl.quantize_encrypt(w, device=False, normalize=True, degree=bad)
        assert _state(cl) == before and all(w._weights[k] is layers[k] for k in layers), repr(bad)
    ref, got, agg = _round(5000.0)
    before = _state(got)
    w = _W({"a": agg.copy()})
    cases = [dict(degree=bad, total_degree=10.0) for bad in BAD] + [dict(degree=5.0, total_degree=bad) for bad in BAD]
    cases += [dict(degree=5.0)]                                   # a degree without a total_degree
    for kw in cases:
        with pytest.raises(ValueError):
            got.decrypt_unquantize(w, **kw)
        with pytest.raises(ValueError):
            got.decrypt_unquantize(w, out={}, **kw)
        assert _state(got) == before and list(w._weights) == ["a"], kw
    got.degree = None
    with pytest.raises(ValueError):
        got.decrypt_unquantize(w, total_degree=10.0)              # a total_degree without any degree
    assert _state(got) == before
    got.degree = 5000.0
    # last_round: host arrays without out=
    tensor = FakeTensor("float32", (129,), 0x7000_0000)
    with pytest.raises(TypeError):
        got.decrypt_unquantize(w, total_degree=10.0, last_round={"a": tensor, "b": np.zeros((3, 43)), "c": np.zeros(33)})
    with pytest.raises(TypeError):
        got.decrypt_unquantize(w, last_round={"a": np.zeros(129)})            # a layer missing
    # tensors on an engine without the new entry points
    outs = {"a": FakeTensor("float32", (129,), 0x5000_0000), "b": FakeTensor("float32", (3, 43), 0x5000_1000), "c": FakeTensor("float32", (33,), 0x5000_2000)}
    with pytest.raises(TypeError):
        got.decrypt_unquantize(w, out=outs, unnormalize=True, total_degree=10.0)
    with pytest.raises(TypeError):
        got.decrypt_unquantize(w, out=outs, last_round=outs)
    with pytest.raises(TypeError):
        got.quantize_encrypt(_W(dict(layers, a=tensor)), degree=5.0)
    assert _state(got)[:6] == before[:6] and list(w._weights) == ["a"]


# ------------------------------------------------------------------------------------------------------------------ the cohorts
class _StageEngine(RecordingEngine):
    limbs = 2

    def stage_layers_dev(self, rows):
        self._rec("stage_layers_dev", list(rows))


def _cohort(monkeypatch, n_local=3):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheCohort
    monkeypatch.setattr(cm.FlasheCipher, "_engine_cls", _StageEngine)
    monkeypatch.setattr(cm, "N_JOBS", 16)
    monkeypatch.setenv("FLASHE_DEVICE_RNG", "0")
    co = FlasheCohort(_args(120, batch=True), first_idx=0, n_local=n_local, num_clients=n_local, prp_seed=KEY)
    co.set_iter_index(4)
    ws = [_W({f"l{i}": np.full(s, 0.01 * (c + 1), np.float32) for i, s in enumerate((7, 0, 50))}) for c in range(n_local)]
    return co, ws


def test_the_cohorts_default_total_degree_is_the_left_to_right_sum(monkeypatch):
    degrees = [0.1, 0.2, 0.3]
    assert (0.1 + 0.2) + 0.3 != 0.1 + (0.2 + 0.3)
    co, ws = _cohort(monkeypatch)
    seen = []
    co.lead.decrypt_unquantize = lambda agg, **kw: seen.append(kw)
    np.random.seed(3)
    co.quantize_encrypt(ws, degrees=degrees)
    co.decrypt_unquantize()
    assert seen[-1]["degree"] == 0.1 and seen[-1]["total_degree"] == functools.reduce(operator.add, degrees) == (0.1 + 0.2) + 0.3
    co.decrypt_unquantize(degree=0.2, total_degree=9.0)
    assert (seen[-1]["degree"], seen[-1]["total_degree"]) == (0.2, 9.0)
    co.decrypt_unquantize(total_degree=9.0)                                   # the lead remembers the first client's
    assert (seen[-1]["degree"], seen[-1]["total_degree"]) == (0.1, 9.0)
    # a round in which client 1 dropped out: the present clients' degrees
    co, ws = _cohort(monkeypatch)
    co.lead.decrypt_unquantize = lambda agg, **kw: seen.append(kw)
    co.quantize_encrypt([ws[0], ws[2]], present=[0, 2], degrees=[0.3, 0.1])
    co.decrypt_unquantize()
    assert (seen[-1]["degree"], seen[-1]["total_degree"]) == (0.3, 0.3 + 0.1)
    # without degrees nothing is handed on
    co, ws = _cohort(monkeypatch)
    co.lead.decrypt_unquantize = lambda agg, **kw: seen.append(kw)
    co.quantize_encrypt(ws)
    co.decrypt_unquantize()
    assert (seen[-1]["degree"], seen[-1]["total_degree"]) == (None, None)


def test_degrees_of_another_length_or_value_are_refused_before_anything_is_touched(monkeypatch):
    co, ws = _cohort(monkeypatch)
    q, eng = co.lead.quantizer, co.cipher.engine
    np.random.seed(5)
    st = np.random.get_state()
    co._last, co._degrees = "last", "degrees"
    before = (q.alpha_list, q.r_max_list, q.layer_size_list)
    for bad in ([1.0, 2.0], [1.0, 2.0, 3.0, 4.0], [], [1.0, 0.0, 2.0], [1.0, None, 2.0], [1.0, "2", 3.0], [1.0, float("nan"), 3.0]):
        with pytest.raises(ValueError):
            co.quantize_encrypt(ws, degrees=bad)
        now = np.random.get_state()
        assert (q.alpha_list, q.r_max_list, q.layer_size_list) == before and eng.log == [] and co._last == "last" and co._degrees == "degrees"
        assert now[1].tobytes() == st[1].tobytes() and now[2] == st[2]
    with pytest.raises(ValueError):
        co.quantize_encrypt(ws[:2], present=[0, 2], degrees=[1.0, 2.0, 3.0])
    for kw in (dict(degree=1.0), dict(total_degree=0.0), dict(degree=-1.0, total_degree=2.0)):
        with pytest.raises(ValueError):
            co.decrypt_unquantize(aggregate=np.zeros((4, 2), np.uint64), **kw)


def test_the_plan_and_the_launches_are_the_same_with_and_without_degrees(monkeypatch):
    # host layers are multiplied on the host: the planner's answer, the path and the engine calls do not change
    co_a, ws = _cohort(monkeypatch)
    co_b, _ws = _cohort(monkeypatch)
    pa, pb = co_a.plan(ws), co_b.plan(ws)
    np.random.seed(3)
    ua = co_a.quantize_encrypt(ws)
    np.random.seed(3)
    ub = co_b.quantize_encrypt(ws, degrees=[5000.0, 3, np.float32(0.3)], normalize=False)
    assert (pa.path, pa.reason, pa.n, pa.n_elems, pa.names, pa.sizes) == (pb.path, pb.reason, pb.n, pb.n_elems, pb.names, pb.sizes)
    assert ua.path == ub.path == pa.path and co_a.cipher.engine.log == co_b.cipher.engine.log
    assert "stage_layers_dev" not in co_b.cipher.engine.log
    # degrees of mixed scalar types make a float32 layer float64 for some clients only: the existing "mixed" rule sends it to the staged form
    co_c, _ws = _cohort(monkeypatch)
    uc = co_c.quantize_encrypt(ws, degrees=[5000.0, np.float64(37.0), 3])
    assert uc.path == "staged-chain"


def test_the_sparse_cohort_hands_the_three_arguments_to_its_lead(monkeypatch):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheSparseCohort
    monkeypatch.setattr(cm.FlasheCipher, "_engine_cls", _StageEngine)
    co = FlasheSparseCohort(dict(_args(20), mask="dynamic"), first_idx=0, n_local=2, num_clients=2, prp_seed=KEY, sparsity=0.1)
    for kw in (dict(degree=1.0), dict(total_degree=-2.0), dict(degree=0, total_degree=2.0)):
        with pytest.raises(ValueError, match="degree"):
            co.decrypt_unquantize(aggregate=np.zeros(4, np.uint64), **kw)
