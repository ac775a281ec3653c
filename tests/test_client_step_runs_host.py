"""CPU test of the one loop in FlasheClient's fused step that no other test reaches (flashe_amd/block.py, _encrypt_tail): the model cut into
runs of whole layers of at most _RNG_RUN_MAX draws (2^26 in production, 5 here), one draw call and one launch per run, for host layers
(*_model_dev) and for framework tensors (*_tensors_dev), and the sparse job's trailing 'zzz' value behind them.  On the recording engine
of tests/trace_client_step.py; touches no device."""
import numpy as np
import pytest

import trace_client_step as T
from flashe_amd import block, quantize

SIZES = [4, 3, 0, 6, 2]                    # 6 > 5: a lone layer over the cap; 0: an empty layer
RUNS = [(0, 4), (4, 3), (7, 6), (13, 2)]
N = sum(SIZES)


def _state():
    st = np.random.get_state()
    return st[0], st[1].tobytes(), st[2]


@pytest.fixture
def client(monkeypatch):
    T.install(monkeypatch)
    monkeypatch.setattr(block, "_RNG_RUN_MAX", 5)
    monkeypatch.setenv("FLASHE_DEVICE_RNG", "0")

    def make(int_bits):
        cl = T.make_client(int_bits)
        np.random.seed(23)
        return cl, cl.cipher.engine
    return make


def _host():
    return {f"l{i}": np.linspace(-1, 1, s).astype(np.float32) for i, s in enumerate(SIZES)}


def _tensors():
    return {f"l{i}": T.FakeTensor(["float32", "float64", "float16"][i % 3], (s,), 0x7000_0000 + 4096 * i) for i, s in enumerate(SIZES)}


def _check_runs(eng, ct, launch, n_draws=N):
    calls = [a for name, a, _kw in eng.calls if name == launch]
    assert [(a[5], a[6]) for a in calls] == RUNS                               # one launch per run: (first, count)
    ups = [a for name, a, _kw in eng.calls if name == "upload" and a[0].dtype == np.float64]
    assert [u[0].size for u in ups] == [c for _f, c in RUNS]
    for a, u in zip(calls, ups):
        assert a[9] is u[1]                                                    # the run's own draws
        assert a[10] == ct.ptr + a[5] * eng.limbs * 8                          # written at the run's first element
        assert a[3] == N and a[7] == calls[0][7] and [r[0] for r in a[7]] == [0, 4, 7, 7, 13]       # n and the table: the whole model's
    after = _state()
    np.random.seed(23)
    want = np.random.random(n_draws)
    assert np.array_equal(np.concatenate([u[0] for u in ups]), want[:N])       # flat element j takes draw j
    assert _state() == after                                                   # and the stream stands where one such call leaves it
    return want


@pytest.mark.parametrize("int_bits", [128, 20])
def test_host_layers_take_one_launch_per_run(client, int_bits):
    cl, eng = client(int_bits)
    res = cl.quantize_encrypt(T.W(_host()))
    ct = res._weights["l0"]
    assert len(ct) == N and list(res._weights) == ["l0"]
    _check_runs(eng, ct, "quantize_encrypt_model_dev")
    assert not [name for name, _a, _kw in eng.calls if name in ("hold", "quantize_encrypt_tensors_dev")]
    assert cl.shape_dict == {f"l{i}": (s,) for i, s in enumerate(SIZES)} and len(cl.quantizer.alpha_list) == 5


@pytest.mark.parametrize("int_bits", [128, 20])
def test_tensor_layers_take_the_same_runs_and_one_hold(client, int_bits):
    cl, eng = client(int_bits)
    layers = _tensors()
    res = cl.quantize_encrypt(T.W(layers))
    ct = res._weights["l0"]
    assert len(ct) == N
    _check_runs(eng, ct, "quantize_encrypt_tensors_dev")
    holds = [a for name, a, _kw in eng.calls if name == "hold"]
    assert len(holds) == 1 and len(holds[0][0]) == 5
    assert not [name for name, _a, _kw in eng.calls if name == "quantize_encrypt_model_dev"]
    table = [a for name, a, _kw in eng.calls if name == "quantize_encrypt_tensors_dev"][0][7]
    assert [r[1] for r in table] == [layers[f"l{i}"].ptr for i in range(5)] and all(len(r) == 6 for r in table)


@pytest.mark.parametrize("int_bits", [128, 20])
@pytest.mark.parametrize("tensors", [False, True])
def test_the_sparse_jobs_zzz_value_takes_the_draw_after_the_models(client, int_bits, tensors):
    cl, eng = client(int_bits)
    layers = _tensors() if tensors else _host()
    layers["zzz"] = np.array([0.25], dtype=np.float32)
    res = cl.quantize_encrypt(T.W(layers))
    ct = res._weights["l0"]
    assert list(res._weights) == ["l0"] and len(ct) == N + 1                    # the un-encrypted value closes the upload
    want = _check_runs(eng, ct, "quantize_encrypt_tensors_dev" if tensors else "quantize_encrypt_model_dev", n_draws=N + 1)
    zq = [a for name, a, _kw in quantize._engines[(64, 0)].calls if name == "quantize"]
    assert len(zq) == 1 and zq[0][1] == 1.0 and np.array_equal(zq[0][3], want[N:])      # alpha 1.0, the 16th draw
    tail = [a for name, a, _kw in eng.calls if name == "buf.upload_at" and a[0] is ct.buf]
    assert len(tail) == 1 and tail[0][1] == N * eng.limbs * 8 and tail[0][2].size == eng.limbs
    assert "zzz" not in cl.shape_dict and len(cl.shape_dict) == 5
