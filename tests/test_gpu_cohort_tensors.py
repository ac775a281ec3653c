"""GPU: FlasheCohort on a training framework's tensors -- mixed host / device layers in four dtypes, the full-size ten-client round with
nothing but tables crossing PCIe, stream order, lifetime and the refusals -- bit for bit against FlasheClients run one after the other."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEY = bytes(range(32))
IT = 5
ARGS = {"quantize": {"int_bits": 128, "batch": False, "element_bits": 16, "padding": True, "secure": True}, "precompute": {"enable": False}}
FULL_SIZES = [9408] + [s for s in (4096, 16384, 36864, 65536, 147456, 262144, 589824, 1048576, 2359296) for _ in range(6)] + [2048000, 1000]


class _W:
    def __init__(self, layers):
        self.walking_order = sorted(layers)
        self._weights = dict(layers)


# (imported when the module is collected: a torch that comes into the process after the engine has started work may not see the GPU)
torch_mod = pytest.importorskip("torch")


def _torch():
    torch = torch_mod
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible to torch")
    return torch


def _client(idx, C, stream=None):
    from flashe_amd.block import FlasheClient
    cl = FlasheClient(ARGS, stream=stream)
    cl.create_cipher(idx, C, KEY)
    cl.set_iter_index(IT)
    return cl


def _cohort(C, stream=None, first_idx=0, num_clients=None):
    from flashe_amd.block import FlasheCohort
    co = FlasheCohort(ARGS, first_idx=first_idx, n_local=C, num_clients=C if num_clients is None else num_clients, prp_seed=KEY, stream=stream)
    co.set_iter_index(IT)
    return co


def _admission():
    from flashe_amd import Engine
    from flashe_amd.block import cohort_admission_length
    return cohort_admission_length(Engine(KEY, 128).cu_count)


def _same_state(a, b):
    return a[0] == b[0] and a[2] == b[2] and np.array_equal(a[1], b[1])


def _mixed_models(torch, C, n, seed):
    """Per client the same eight layers: host float32 / float64 and device float32 / float64 / float16 / bfloat16, sizes with a single
    value, an odd prime, an end in the middle of a tile and an empty layer."""
    sizes = [1, 10007, 256 * 21 + 77, 0, 300001, 65536]
    sizes += [(n - sum(sizes)) // 2]
    sizes += [n - sum(sizes)]
    kinds = ["dev:float32", "host:float64", "dev:bfloat16", "dev:float32", "dev:float16", "host:float32", "dev:float64", "dev:float32"]
    g = torch.Generator(device="cuda").manual_seed(seed)
    models = []
    for c in range(C):
        m = {}
        for i, (s, kind) in enumerate(zip(sizes, kinds)):
            where, dt = kind.split(":")
            t = (torch.randn((s,) if i % 2 else (s, 1), generator=g, device="cuda", dtype=torch.float64) * 0.05 + 0.002 * c).to(getattr(torch, dt))
            m[f"l{i}"] = t if where == "dev" else t.cpu().numpy()
        models.append(m)
    return models


@pytest.mark.parametrize("C, normalize", [(2, True), (10, False)])
def test_mixed_layers_three_rounds_into_model_tensors(C, normalize):
    torch = _torch()
    from flashe_amd import cipher as cm
    cm.N_JOBS = 16
    n = _admission() + 4321
    clients = [_client(c, C) for c in range(C)]
    co = _cohort(C)
    for it in range(3):
        for cl in clients:
            cl.set_iter_index(it)
        co.set_iter_index(it)
        models = _mixed_models(torch, C, n, 40 + it)
        np.random.seed(it)
        np.random.random(5)
        state = np.random.get_state()
        want = []
        for cl, m in zip(clients, models):
            w = cl.quantize_encrypt(_W(dict(m)), device=True, normalize=normalize)
            want.append(w._weights[w.walking_order[0]])
        want_state = np.random.get_state()
        want_sum = clients[0].cipher.aggregate(want)
        np.random.set_state(state)
        up = co.quantize_encrypt([_W(dict(m)) for m in models], normalize=normalize)
        assert up.path == "cohort-chain"
        assert _same_state(np.random.get_state(), want_state)
        for c in range(C):
            assert up.ciphertexts[c].to_host().tobytes() == want[c].to_host().tobytes(), (it, c)
        assert up.partial_sum.to_host().tobytes() == want_sum.to_host().tobytes()
        # both sides decrypt into tensors of the layers' own dtypes (host layers: float64 tensors)
        def outs():
            return {k: torch.full(tuple(np.shape(v)) if isinstance(v, np.ndarray) else tuple(v.shape), float("nan"), device="cuda",
                                  dtype=torch.float64 if isinstance(v, np.ndarray) else v.dtype) for k, v in models[0].items()}
        ref_out, got_out = outs(), outs()
        clients[0].set_idx_list(list(range(C)))
        clients[0].decrypt_unquantize(_W({"l0": want_sum}), out=ref_out, unnormalize=True)
        got = co.decrypt_unquantize(out=got_out, unnormalize=True)
        for k in ref_out:
            assert got._weights[k] is got_out[k]
            assert torch.equal(ref_out[k].view(torch.uint8), got_out[k].view(torch.uint8)), (it, k)
        qa, qb = co.quantizer, clients[0].quantizer
        assert [float(x).hex() for x in qa.past_layer_mean_list] == [float(x).hex() for x in qb.past_layer_mean_list]
        assert [float(x).hex() for x in qa.past_layer_std_list] == [float(x).hex() for x in qb.past_layer_std_list]
        for cl in clients[1:]:
            cl.quantizer.past_layer_mean_list = list(qb.past_layer_mean_list)
            cl.quantizer.past_layer_std_list = list(qb.past_layer_std_list)


def test_full_size_ten_client_round_stays_on_the_device(monkeypatch):
    """Ten float32 copies of the 57-layer, 29.2 M-parameter model with different values: every ciphertext and the sum against the
    sequential steps, the decrypted model against a client's, and no ciphertext, draw or layer over PCIe in the cohort's round (the
    tables of ten 57-layer clients and the statistics are a few KB; NumPy's MT19937 state is in use, so the draws are made on the device)."""
    torch = _torch()
    from flashe_amd import cipher as cm
    from flashe_amd import engine as E
    cm.N_JOBS = 16
    C = 10
    g = torch.Generator(device="cuda").manual_seed(9)
    models = [{f"l{i:03d}": torch.randn(s, generator=g, device="cuda") * 0.05 + 0.001 * c for i, s in enumerate(FULL_SIZES)} for c in range(C)]
    clients = [_client(c, C) for c in range(C)]
    np.random.seed(11)
    state = np.random.get_state()
    want = []
    for cl, m in zip(clients, models):
        w = cl.quantize_encrypt(_W(dict(m)), device=True, normalize=True)
        want.append(w._weights[w.walking_order[0]])
    want_state = np.random.get_state()
    want_sum = clients[0].cipher.aggregate(want)
    ref_out = {k: torch.empty_like(t) for k, t in models[0].items()}
    clients[0].set_idx_list(list(range(C)))
    clients[0].decrypt_unquantize(_W({"l000": want_sum}), out=ref_out, unnormalize=True)
    co = _cohort(C)
    moved = [0]

    def counting(fn, size_of):
        def wrap(*a, **kw):
            r = fn(*a, **kw)
            moved[0] += size_of(a, kw, r)
            return r
        return wrap

    with monkeypatch.context() as mp:
        mp.setattr(E.Engine, "upload", counting(E.Engine.upload, lambda a, kw, r: np.asarray(a[1]).nbytes))
        mp.setattr(E.DeviceBuffer, "upload", counting(E.DeviceBuffer.upload, lambda a, kw, r: np.asarray(a[1]).nbytes))
        mp.setattr(E.DeviceBuffer, "upload_at", counting(E.DeviceBuffer.upload_at, lambda a, kw, r: np.asarray(a[2]).nbytes))
        mp.setattr(E.DeviceBuffer, "download", counting(E.DeviceBuffer.download, lambda a, kw, r: r.nbytes))
        mp.setattr(E.DeviceBuffer, "download_at", counting(E.DeviceBuffer.download_at, lambda a, kw, r: r.nbytes))
        np.random.set_state(state)
        up = co.quantize_encrypt([_W(dict(m)) for m in models], normalize=True)
        got_out = {k: torch.full_like(t, float("nan")) for k, t in models[0].items()}
        co.decrypt_unquantize(out=got_out, unnormalize=True)
        assert moved[0] < 64 * 1024, moved[0]
    assert up.path == "cohort-chain"
    assert _same_state(np.random.get_state(), want_state)
    for c in range(C):
        assert up.ciphertexts[c].to_host().tobytes() == want[c].to_host().tobytes(), c
    assert up.partial_sum.to_host().tobytes() == want_sum.to_host().tobytes()
    for k in ref_out:
        assert torch.equal(ref_out[k].view(torch.uint8), got_out[k].view(torch.uint8)), k
    assert [float(x).hex() for x in co.quantizer.past_layer_std_list] == [float(x).hex() for x in clients[0].quantizer.past_layer_std_list]


# ---------------------------------------------------------------- stream order, lifetime, refusals
def _plain_models(torch, C, n, seed, dtype="float32"):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [{"a": (torch.randn(n - 1000, generator=g, device="cuda") * 0.05).to(getattr(torch, dtype)),
             "b": (torch.randn((10, 100), generator=g, device="cuda") * 0.05 + 0.01 * c).to(getattr(torch, dtype))} for c in range(C)]


def _reference(torch, models, C, stream=None):
    clients = [_client(c, C, stream=stream) for c in range(C)]
    cts = []
    for cl, m in zip(clients, models):
        w = cl.quantize_encrypt(_W({k: t.clone() for k, t in m.items()}), device=True)
        cts.append(w._weights[w.walking_order[0]])
    agg = clients[0].cipher.aggregate(cts)
    out = {k: torch.empty_like(t) for k, t in models[0].items()}
    clients[0].set_idx_list(list(range(C)))
    clients[0].decrypt_unquantize(_W({"a": agg}), out=out)
    torch.cuda.synchronize()
    return [c.to_host().tobytes() for c in cts], agg.to_host().tobytes(), out


def test_tensors_freed_right_after_the_call():
    """Own-stream mode: the caller drops (and overwrites the memory of) its tensors as soon as the call returns."""
    torch = _torch()
    from flashe_amd import cipher as cm
    cm.N_JOBS = 16
    C, n = 3, _admission() + 10
    models = _plain_models(torch, C, n, 3, "bfloat16")
    np.random.seed(21)
    want_cts, want_sum, _o = _reference(torch, models, C)
    co = _cohort(C)
    np.random.seed(21)
    torch.cuda.synchronize()
    up = co.quantize_encrypt([_W({k: t.clone() for k, t in m.items()}) for m in models])      # the clones die with the call
    junk = [torch.full((n,), 7.0, device="cuda", dtype=torch.bfloat16) for _ in range(2 * C)]  # the allocator may hand their memory out again
    assert up.path == "cohort-chain"
    assert [c.to_host().tobytes() for c in up.ciphertexts] == want_cts and up.partial_sum.to_host().tobytes() == want_sum
    del junk


def test_shared_stream_mode_is_ordered_with_the_framework():
    torch = _torch()
    from flashe_amd import cipher as cm
    cm.N_JOBS = 16
    C, n = 2, _admission() + 10
    models = _plain_models(torch, C, n, 4)
    np.random.seed(22)
    want_cts, want_sum, want_out = _reference(torch, models, C)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        co = _cohort(C, stream=side.cuda_stream)
        staged = [{k: torch.empty_like(t) for k, t in m.items()} for m in models]
        torch.cuda._sleep(100_000_000)                        # the copies below are still queued when the cohort is called
        for s, m in zip(staged, models):
            for k in m:
                s[k].copy_(m[k], non_blocking=True)
        np.random.seed(22)
        up = co.quantize_encrypt([_W(dict(s)) for s in staged])
        out = {k: torch.full_like(t, float("nan")) for k, t in models[0].items()}
        co.decrypt_unquantize(out=out)
        same = [bool(torch.equal(out[k].view(torch.uint8), want_out[k].view(torch.uint8))) for k in out]     # read on the same stream, no host sync
    assert up.path == "cohort-chain" and all(same)
    assert [c.to_host().tobytes() for c in up.ciphertexts] == want_cts and up.partial_sum.to_host().tobytes() == want_sum


def test_refusals_come_before_any_launch(monkeypatch):
    torch = _torch()
    from flashe_amd import cipher as cm
    from flashe_amd import engine as E
    cm.N_JOBS = 16
    C, n = 2, _admission() + 10
    co = _cohort(C)
    launched = []
    for name in ("numpy_random_dev", "quantize_encrypt_cohort_dev", "quantize_batch_tensors_dev", "encrypt_batch_sum_dev", "combine_unquantize_model_dev",
                 "decrypt_unquantize_model_dev", "store_layers_dev", "alloc"):
        fn = getattr(E.Engine, name)
        monkeypatch.setattr(E.Engine, name, (lambda f, nm: lambda *a, **kw: (launched.append(nm), f(*a, **kw))[1])(fn, name))
    good = lambda: {"a": torch.zeros(n - 8, device="cuda"), "b": torch.zeros((2, 4), device="cuda")}      # noqa: E731
    bad_grad = good()
    bad_grad["b"] = torch.zeros((2, 4), device="cuda", requires_grad=True)
    with pytest.raises(BufferError, match="require gradient"):
        co.quantize_encrypt([_W(good()), _W(bad_grad)])
    bad_strides = good()
    bad_strides["b"] = torch.zeros((4, 2), device="cuda").T
    with pytest.raises(ValueError, match="C-contiguous"):
        co.quantize_encrypt([_W(good()), _W(bad_strides)])
    bad_dtype = good()
    bad_dtype["b"] = torch.zeros((2, 4), device="cuda", dtype=torch.int32)
    with pytest.raises(TypeError, match="unsupported dtype"):
        co.quantize_encrypt([_W(good()), _W(bad_dtype)])
    bad_host = good()
    bad_host["b"] = torch.zeros((2, 4))                       # a CPU tensor is not ROCm device memory
    with pytest.raises(ValueError, match="ROCm device memory"):
        co.quantize_encrypt([_W(good()), _W(bad_host)])
    if torch.cuda.device_count() >= 2:
        other = good()
        other["b"] = torch.zeros((2, 4), device="cuda:1")
        with pytest.raises(ValueError, match="device 1, this engine on device 0"):
            co.quantize_encrypt([_W(good()), _W(other)])
    assert launched == [], launched
    np.random.seed(1)
    up = co.quantize_encrypt([_W(good()), _W(good())])
    assert up.path == "cohort-chain"
    del launched[:]
    with pytest.raises(ValueError, match="expected shape"):
        co.decrypt_unquantize(out={"a": torch.zeros(n - 8, device="cuda"), "b": torch.zeros((4, 2), device="cuda")})
    with pytest.raises(TypeError, match="unsupported dtype"):
        co.decrypt_unquantize(out={"a": torch.zeros(n - 8, device="cuda"), "b": torch.zeros((2, 4), device="cuda", dtype=torch.int32)})
    with pytest.raises(KeyError):
        co.decrypt_unquantize(out={"a": torch.zeros(n - 8, device="cuda")})
    assert launched == [], launched
    out = {"a": torch.empty(n - 8, device="cuda"), "b": torch.empty((2, 4), device="cuda")}
    co.decrypt_unquantize(out=out)
    assert "combine_unquantize_model_dev" in launched and bool(torch.isfinite(out["a"]).all())
