"""GPU: a cohort of sparse-job clients on one card (flashe_amd.block.FlasheSparseCohort) against the reference's recorded steps
(clientstep.json, sparsify.json) and against the same clients run one after the other as Sparsifier + FlasheClient in one process --
packed locations, compact values, residuals, uploads, their dense aggregate, NumPy's generator, the decrypted floats and the
quantiser's history, compared as bytes.  `up.path` is asserted in every case so that a silent mis-route shows; output blocks are
poisoned first."""
import numpy as np
import pytest

from conftest import load_golden, unhex

pytestmark = pytest.mark.gpu

KEY = bytes(range(32))

try:
    # (asked at collection: once a test has created an engine, the framework of the same process no longer finds its device)
    import torch as _torch_mod
    _TORCH_GPU = _torch_mod.cuda.is_available()
except ImportError:
    _TORCH_GPU = False


class _W:
    def __init__(self, layers):
        self.walking_order = sorted(layers, key=str)
        self._weights = dict(layers)


def _torch():
    torch = pytest.importorskip("torch")
    if not (_TORCH_GPU and torch.cuda.is_available()):
        pytest.skip("no GPU visible to torch")
    return torch


def _args(b, eb=16, batch=False, precompute=False):
    return {"quantize": {"int_bits": b, "batch": batch, "element_bits": eb, "padding": True, "secure": True},
            "precompute": {"enable": precompute, "num_params": 11}, "mask": "dynamic"}


def _poison(eng, sizes):
    """Blocks of the sizes the next call allocates, filled with a pattern and handed back to the engine's pool."""
    bufs = [eng.alloc(s) for s in sizes]
    for b, s in zip(bufs, sizes):
        eng.memset_dev(b, 0xA5, s)
    eng.sync()
    for b in bufs:
        b.free()


def _poison_round(co, K, total):
    lim = co.engine.limbs
    _poison(co.engine, [8 * lim * (K + 1)] * co.n_local + [8 * lim * total, ((8 * K + 15) & ~15) * co.n_local, 8 * total])


def _same_state(a, b):
    return a[0] == b[0] and a[2] == b[2] and np.array_equal(a[1], b[1])


def _host(t):
    import torch
    return (t.float() if t.dtype in (torch.float16, torch.bfloat16) else t).cpu().numpy()


def _is_tensor(v):
    return not isinstance(v, np.ndarray)


# ------------------------------------------------------------------------------------------------ 1. the reference's recorded steps
@pytest.mark.parametrize("form", ["host", "tensor"])
@pytest.mark.parametrize("case_i", [0, 1])
def test_the_reference_jobs_sparse_client_steps(case_i, form):
    """Both sparse cases of clientstep.json (b = 128, C = 3; b = 64, C = 2) through dynamic_masking(choice, masks, total) +
    quantize_encrypt(compact=, seeds=): every upload, the aggregate, alpha_list and decrypt_unquantize's floats equal the fixture."""
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheSparseCohort
    from oracle.flashe_oracle import limbs_to_ints
    torch = _torch() if form == "tensor" else None
    case = load_golden("clientstep.json")["sparse"][case_i]
    C = case["num_clients"]
    cm.N_JOBS = case["n_jobs"]
    co = FlasheSparseCohort(_args(case["b"], case["element_bits"]), first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, sparsity=0.1)
    co.set_iter_index(case["iter"])
    assert co.dynamic_masking(case["choice"], case["masks"], case["total"]) == "single"
    compact = []
    for rec in case["clients"]:
        layers = {nm: np.frombuffer(bytes.fromhex(rec["layers"][nm]), dtype=np.dtype(dt)).copy() for nm, _sh, dt in case["dense_layers"]}
        if torch is not None:
            layers = {k: torch.from_numpy(v).cuda() for k, v in layers.items()}
        layers["zzz"] = np.array([0.0])
        compact.append(layers)
    K = sum(case["ks"])
    _poison_round(co, K, case["total"])
    up = co.quantize_encrypt(compact=compact, seeds=[rec["seed"] for rec in case["clients"]])
    assert up.path == "sparse-cohort"
    for c, rec in enumerate(case["clients"]):
        assert len(up.uploads[c]) == K + 1
        assert limbs_to_ints(up.uploads[c].to_host()) == unhex(rec["upload"]), c
        assert [float(a).hex() for a in co.alpha_list] == rec["alpha"]
    assert limbs_to_ints(up.aggregate.to_host()) == unhex(case["agg"])
    co.shape_dict_used_for_sparsification = {nm: tuple(sh) for nm, sh, _dt in case["dense_layers"]}
    if torch is not None:
        outs = {nm: torch.empty(tuple(sh), dtype=torch.float64, device="cuda") for nm, sh, _dt in case["dense_layers"]}
        co.decrypt_unquantize(out=outs)
        got = {k: v.cpu().numpy() for k, v in outs.items()}
    else:
        back = co.decrypt_unquantize()
        got = {k: np.asarray(back._weights[k], dtype=np.float64) for k in back.walking_order}
    for nm, sh, _dt in case["dense_layers"]:
        assert got[nm].shape == tuple(sh)
        assert got[nm].tobytes() == bytes.fromhex(case["unquantized"][nm]), nm


# ------------------------------------------------------------------------------------------------ 2. the reference's sparsifier
@pytest.mark.parametrize("form", ["host", "tensor"])
@pytest.mark.parametrize("C", [1, 3])
def test_sparsify_golden_through_a_cohort(C, form):
    from flashe_amd import weights as wz
    from flashe_amd.block import FlasheSparseCohort
    torch = _torch() if form == "tensor" else None
    for case in load_golden("sparsify.json")["cases"]:
        dt = np.dtype(case["dtype"])
        co = FlasheSparseCohort(_args(128), first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, sparsity=case["sparsity"])
        for rd in case["rounds"]:
            layer = np.frombuffer(bytes.fromhex(rd["layer"]), dtype=dt).copy()
            models = [{"w": torch.from_numpy(layer.copy()).cuda() if torch is not None else layer.copy()} for _ in range(C)]
            enc = co.sparsify(models, ["w"])
            n = layer.size
            want = wz.to_big_int(np.array(rd["location"], dtype=np.uint64), n.bit_length())
            for c in range(C):
                assert enc.encoded[c] == (want[0], len(rd["location"]), n.bit_length(), n), c
                buf, k = enc.locations[c]
                assert k == len(rd["location"]) and buf.download_at(0, np.uint32, k).tolist() == rd["location"]
                assert enc.compact[c]["w"].to_host().tobytes().hex() == rd["masked"]
                r = co.remain_weights(c)["w"]
                assert r.dtype == dt and r.tobytes().hex() == rd["remain"]
                if torch is not None:
                    assert torch.equal(models[c]["w"], torch.from_numpy(layer).cuda())
                else:
                    assert models[c]["w"].tobytes() == layer.tobytes()
        assert co.shape_dict_used_for_sparsification == {"w": (n,)}


# ------------------------------------------------------------------------------------------------ 3. against the sequential clients
SIZES = [1, 10007, 256 * 37 + 91, 4099, 400_003, 1, 1023, 70_001, 150_000]      # one-value layers, a prime, sizes that end mid-tile
NAMES = [f"l{i:02d}" for i in range(len(SIZES))]


def _models(C, sizes, seed, dtypes, torch=None, host_layers=()):
    """C models of len(sizes) layers; dtypes cycle over the layers; with torch the layers are device tensors except `host_layers`."""
    g = np.random.Generator(np.random.PCG64(seed))
    out = []
    for c in range(C):
        m = {}
        for i, s in enumerate(sizes):
            name, dn = f"l{i:02d}", dtypes[i % len(dtypes)]
            x = g.standard_normal(s) * 0.05 + 0.01 * c
            shape = (s,) if i % 2 else (1, s)
            if torch is None or i in host_layers:
                m[name] = x.astype(np.float64 if dn == "float64" else np.float32).reshape(shape)
            else:
                tdt = {"float32": torch.float32, "float64": torch.float64, "float16": torch.float16, "bfloat16": torch.bfloat16}[dn]
                m[name] = torch.from_numpy(x).to(tdt).reshape(shape).cuda()
        out.append(m)
    return out


def _hostified(m):
    return {k: (_host(v) if _is_tensor(v) else v) for k, v in m.items()}


class _Sequential:
    """num_clients Sparsifiers + FlasheClients of one process; client 0's refreshed mean / std lists are copied to the others after
    each round (every client's history derives from the same global model)."""

    def __init__(self, b, sparsity, num_clients, total):
        from flashe_amd.block import FlasheClient
        from flashe_amd.weights import Sparsifier
        self.cls, self.sps, self.total = [], [], total
        for c in range(num_clients):
            cl = FlasheClient(_args(b))
            cl.create_cipher(c, num_clients, KEY)
            cl.cipher.total = total
            self.cls.append(cl)
            self.sps.append(Sparsifier(sparsity))

    def sparsify(self, models, names):
        from flashe_amd.weights import from_big_int
        self.encs, self.masks, self.compact = [], [], []
        for sp, m in zip(self.sps, models):
            w = _hostified(m)
            enc = sp.sparsify(w, names)
            self.encs.append(enc)
            self.masks.append(np.asarray(from_big_int(enc[0], enc[1], enc[2], as_object=False)).astype(np.int64).reshape(-1))
            self.compact.append(w)

    def step(self, it, choice, normalize, state=None, seeds=None, who=None):
        if state is not None:
            np.random.set_state(state)
        self.uploads = []
        for c, cl in enumerate(self.cls):
            if who is not None and c not in who:
                self.uploads.append(None)
                continue
            cl.set_iter_index(it)
            cl.dynamic_masking(choice, self.masks)
            w = _W(dict(self.compact[c]))
            w._weights["zzz"] = np.array([0.0])
            w.walking_order = sorted(w._weights, key=str)
            if seeds is not None:
                np.random.seed(seeds[c])
            out = cl.quantize_encrypt(w, device=True, normalize=normalize)
            self.uploads.append(out._weights[out.walking_order[0]])
        return np.random.get_state()

    def aggregate(self, who):
        from flashe_amd.block import aggregate_sparse_uploads
        return aggregate_sparse_uploads(self.cls[who[0]].cipher.engine, [self.uploads[c] for c in who], [self.masks[c] for c in who], self.total, device=True)

    def decrypt(self, c, agg, names, unnormalize):
        cl = self.cls[c]
        cl.set_idx_list(list(range(len(self.cls))))
        cl.shape_dict = dict(self.sps[c].shape_dict_used_for_sparsification)
        back = cl.decrypt_unquantize(_W({names[0]: agg}), unnormalize=unnormalize)
        for other in self.cls:
            other.quantizer.past_layer_mean_list = list(cl.quantizer.past_layer_mean_list)
            other.quantizer.past_layer_std_list = list(cl.quantizer.past_layer_std_list)
        return {k: np.asarray(back._weights[k]) for k in names}


def _hexes(vals):
    return [float(v).hex() for v in vals]


def _rounds(C, sizes, b, sparsity, normalize, dtypes, rounds=3, torch=None, host_layers=(), seed=40):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheSparseCohort
    cm.N_JOBS = 16
    names = [f"l{i:02d}" for i in range(len(sizes))]
    total = sum(sizes)
    seq = _Sequential(b, sparsity, C, total)
    co = FlasheSparseCohort(_args(b), first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, sparsity=sparsity)
    for it in range(1, rounds + 1):
        models = _models(C, sizes, seed + it, dtypes, torch, host_layers)
        before = [{k: (v.clone() if _is_tensor(v) else v.copy()) for k, v in m.items()} for m in models]
        seq.sparsify(models, names)
        enc = co.sparsify(models, names)
        K = enc.encoded[0][1]
        for c in range(C):
            assert enc.encoded[c] == seq.encs[c], (it, c)
            buf, k = enc.locations[c]
            assert k == K and np.array_equal(buf.download_at(0, np.uint32, k), seq.masks[c].astype(np.uint32)), (it, c)
            for nm in names:
                h = np.asarray(seq.compact[c][nm])
                assert enc.compact[c][nm].dtype == h.dtype and enc.compact[c][nm].to_host().tobytes() == h.tobytes(), (it, c, nm)
                if _is_tensor(models[c][nm]):
                    assert torch.equal(models[c][nm], before[c][nm]), (it, c, nm)
                else:
                    assert models[c][nm].tobytes() == before[c][nm].tobytes(), (it, c, nm)
        assert co.shape_dict_used_for_sparsification == {nm: tuple(models[0][nm].shape) for nm in names}
        co.set_iter_index(it)
        choice = co.dynamic_masking()
        from flashe_amd.block import dynamic_masking_choice
        assert choice == dynamic_masking_choice(seq.masks, total) == "single"
        np.random.seed(1000 * seed + it)
        state = np.random.get_state()
        st_seq = seq.step(it, choice, normalize, state=state)
        np.random.set_state(state)
        _poison_round(co, K, total)
        up = co.quantize_encrypt(normalize=normalize)
        assert up.path == "sparse-cohort"
        assert _same_state(np.random.get_state(), st_seq), it
        for c in range(C):
            assert np.array_equal(up.uploads[c].to_host(), seq.uploads[c].to_host()), (it, c)
        agg = seq.aggregate(list(range(C)))
        assert np.array_equal(up.aggregate.to_host(), agg.to_host()), it
        assert _hexes(co.alpha_list) == _hexes(seq.cls[0].quantizer.alpha_list)
        assert co.shape_dict == seq.cls[0].shape_dict
        want = seq.decrypt(0, agg, names, normalize)
        if torch is not None:
            outs = {nm: torch.empty(tuple(models[0][nm].shape), dtype=torch.float64, device="cuda") for nm in names}
            co.decrypt_unquantize(out=outs, unnormalize=normalize)
            got = {k: v.cpu().numpy() for k, v in outs.items()}
        else:
            back = co.decrypt_unquantize(unnormalize=normalize)
            got = {k: np.asarray(back._weights[k]) for k in names}
        for nm in names:
            assert got[nm].dtype == want[nm].dtype and got[nm].shape == want[nm].shape and got[nm].tobytes() == want[nm].tobytes(), (it, nm)
        assert _hexes(co.quantizer.past_layer_mean_list) == _hexes(seq.cls[0].quantizer.past_layer_mean_list), it
        assert _hexes(co.quantizer.past_layer_std_list) == _hexes(seq.cls[0].quantizer.past_layer_std_list), it
    for c in range(C):
        a, r = co.remain_weights(c), seq.sps[c].remain_weights
        assert a.keys() == r.keys()
        for nm in names:
            assert a[nm].dtype == np.asarray(r[nm]).dtype and a[nm].tobytes() == np.asarray(r[nm]).tobytes(), (c, nm)


def test_ten_host_clients_b20_mixed_float32_float64_normalised():
    _rounds(10, SIZES, 20, 0.1, True, ("float32", "float64"))


def test_ten_host_clients_b128_one_percent_not_normalised():
    _rounds(10, SIZES, 128, 0.01, False, ("float32",))


@pytest.mark.parametrize("C", [1, 2])
def test_small_cohorts(C):
    _rounds(C, SIZES, 128, 0.1, True, ("float32", "float64", "float32"))


def test_sixty_five_clients_cross_the_span_pass_group():
    _rounds(65, [1, 1013, 256 * 9 + 17, 30_011], 128, 0.1, True, ("float32",))


def test_ten_float32_tensor_clients():
    torch = _torch()
    _rounds(10, SIZES, 128, 0.1, True, ("float32",), torch=torch)


def test_ten_bfloat16_tensor_clients_b20():
    torch = _torch()
    _rounds(10, SIZES, 20, 0.01, True, ("bfloat16",), torch=torch)


def test_ten_mixed_tensor_clients_with_a_host_layer():
    torch = _torch()
    _rounds(10, SIZES, 128, 0.1, True, ("float32", "bfloat16", "float64", "float16"), torch=torch, host_layers=(3,))


def test_two_resnet50_sized_clients():
    """29.2 M values per model: compact offsets beyond 2^24 and the four-values-per-lane tails at size."""
    sizes = [9408] + [s for s in (4096, 16384, 36864, 65536, 147456, 262144, 589824, 1048576, 2359296) for _ in range(6)] + [2048000, 1001, 1]
    assert sum(sizes) > 29_000_000
    _rounds(2, sizes, 128, 0.1, True, ("float32",), rounds=1)


# ------------------------------------------------------------------------------------------------ 4. a cohort inside a larger federation
def test_a_cohort_inside_a_larger_federation():
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheSparseCohort
    cm.N_JOBS = 16
    N, first, C, b = 9, 3, 4, 128
    sizes = [1, 1013, 256 * 9 + 17, 30_011]
    names, total = [f"l{i:02d}" for i in range(len(sizes))], sum(sizes)
    seq = _Sequential(b, 0.1, N, total)
    co = FlasheSparseCohort(_args(b), first_idx=first, n_local=C, num_clients=N, prp_seed=KEY, sparsity=0.1)
    who = list(range(first, first + C))
    for it in (1, 2):
        models = _models(N, sizes, 70 + it, ("float32", "float64"))
        seq.sparsify(models, names)
        enc = co.sparsify(models[first:first + C], names)
        assert enc.encoded == seq.encs[first:first + C]
        co.set_iter_index(it)
        with pytest.raises(ValueError, match="arbiter"):
            co.dynamic_masking()
        assert co.dynamic_masking("single", [m.tolist() for m in seq.masks], total) == "single"
        seeds = [500 + 10 * it + c for c in range(N)]
        seq.step(it, "single", True, seeds=seeds)
        _poison_round(co, enc.encoded[0][1], total)
        up = co.quantize_encrypt(normalize=True, seeds=seeds[first:first + C])
        assert up.path == "sparse-cohort"
        for i, c in enumerate(who):
            assert np.array_equal(up.uploads[i].to_host(), seq.uploads[c].to_host()), (it, c)
        assert np.array_equal(up.aggregate.to_host(), seq.aggregate(who).to_host()), it
        with pytest.raises(ValueError, match="federation"):
            co.decrypt_unquantize()
        full = seq.aggregate(list(range(N)))
        want = seq.decrypt(first, full, names, True)
        back = co.decrypt_unquantize(full, uploaded=list(range(N)), unnormalize=True)
        for nm in names:
            got = np.asarray(back._weights[nm])
            assert got.dtype == want[nm].dtype and got.tobytes() == want[nm].tobytes(), (it, nm)
        assert _hexes(co.quantizer.past_layer_mean_list) == _hexes(seq.cls[first].quantizer.past_layer_mean_list)
        assert _hexes(co.quantizer.past_layer_std_list) == _hexes(seq.cls[first].quantizer.past_layer_std_list)


# ------------------------------------------------------------------------------------------------ 5. "double" set by hand
def test_double_by_hand_takes_the_per_client_path():
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheSparseCohort
    cm.N_JOBS = 16
    C, b = 3, 128
    sizes = [1, 1013, 256 * 9 + 17, 30_011]
    names, total = [f"l{i:02d}" for i in range(len(sizes))], sum(sizes)
    seq = _Sequential(b, 0.1, C, total)
    co = FlasheSparseCohort(_args(b), first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, sparsity=0.1)
    models = _models(C, sizes, 90, ("float32",))
    seq.sparsify(models, names)
    enc = co.sparsify(models, names)
    assert enc.encoded == seq.encs
    co.set_iter_index(1)
    assert co.dynamic_masking("double", [m.tolist() for m in seq.masks]) == "double"
    np.random.seed(77)
    state = np.random.get_state()
    st_seq = seq.step(1, "double", True, state=state)
    np.random.set_state(state)
    up = co.quantize_encrypt(normalize=True)
    assert up.path == "per-client"
    assert _same_state(np.random.get_state(), st_seq)
    for c in range(C):
        assert np.array_equal(up.uploads[c].to_host(), seq.uploads[c].to_host()), c
    assert np.array_equal(up.aggregate.to_host(), seq.aggregate(list(range(C))).to_host())


# ------------------------------------------------------------------------------------------------ 6. refusals leave no trace
def _trace(co):
    q = co.quantizer
    rem = None if co.remain_weights(0) is None else [{k: v.tobytes() for k, v in co.remain_weights(c).items()} for c in range(co.n_local)]
    st = np.random.get_state()
    return (st[0], st[1].tobytes(), st[2], rem, _hexes(q.past_layer_mean_list), _hexes(q.past_layer_std_list), q.layer_size_list and list(q.layer_size_list))


def test_refusals_leave_no_trace():
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheSparseCohort
    cm.N_JOBS = 16
    C, b = 3, 128
    sizes = [1, 1013, 256 * 9 + 17]
    names = [f"l{i:02d}" for i in range(len(sizes))]
    co = FlasheSparseCohort(_args(b), first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, sparsity=0.1)
    models = _models(C, sizes, 5, ("float32",))
    co.set_iter_index(1)
    co.sparsify(models, names)
    co.dynamic_masking()
    np.random.seed(9)
    assert co.quantize_encrypt(normalize=True).path == "sparse-cohort"
    co.decrypt_unquantize(unnormalize=True)
    before = _trace(co)
    bad = [dict(m) for m in _models(C, sizes, 6, ("float32",))]
    bad[2]["l01"] = bad[2]["l01"][:1000]
    with pytest.raises(ValueError, match="client 2: layer 'l01'"):
        co.sparsify(bad, names)
    bad = [dict(m) for m in _models(C, sizes, 6, ("float32",))]
    bad[1]["l02"] = np.zeros((0,), dtype=np.float32)
    with pytest.raises(ValueError):
        co.sparsify(bad, names)
    with pytest.raises(ValueError, match="holds 3 clients"):
        co.sparsify(models[:2], names)
    with pytest.raises(ValueError, match="seeds"):
        co.quantize_encrypt(normalize=True, seeds=[1])
    with pytest.raises(ValueError, match="compact"):
        co.quantize_encrypt(compact=[{}])
    assert _trace(co) == before
    if _TORCH_GPU:
        import torch
        bad = [dict(m) for m in models]
        bad[1]["l01"] = torch.arange(1013, device="cuda", dtype=torch.int32)
        with pytest.raises(TypeError, match="dtype"):
            co.sparsify(bad, names)
        assert _trace(co) == before
        # a batched sparse job does not take tensors: FlasheClient's refusal, before any draw
        cb = FlasheSparseCohort(_args(b, batch=True), first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, sparsity=0.1)
        cb.set_iter_index(1)
        cb.sparsify([{k: torch.from_numpy(v).cuda() for k, v in m.items()} for m in models], names)
        cb.dynamic_masking()
        tb = _trace(cb)
        with pytest.raises(TypeError, match="batched"):
            cb.quantize_encrypt(normalize=True)
        assert _trace(cb) == tb


# ------------------------------------------------------------------------------------------------ 7. PCIe traffic
def test_no_dense_or_compact_layer_data_crosses_pcie(monkeypatch):
    """With tensors a round moves the C packed location integers, the C quantised zeros and the draw rule's uniforms: the one-client
    budget of test_gpu_sparse_tensors.py times C."""
    torch = _torch()
    from flashe_amd import cipher as cm
    from flashe_amd import engine as E
    from flashe_amd.block import FlasheSparseCohort
    from flashe_amd.quantize import DEVICE_RNG_MIN
    cm.N_JOBS = 16
    C = 4
    sizes = {"a": 1_000_000, "b": 600_000, "c": 4099}
    names = sorted(sizes)
    models = [{k: torch.randn(s, device="cuda") for k, s in sizes.items()} for _ in range(C)]
    co = FlasheSparseCohort(_args(128), first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, sparsity=0.01)
    co.set_iter_index(1)
    co.sparsify(models, names)                 # (first call: allocations, tables)
    moved = [0]

    def counting(fn, size_of):
        def wrap(*a, **kw):
            r = fn(*a, **kw)
            moved[0] += size_of(a, kw, r)
            return r
        return wrap

    monkeypatch.setattr(E.DeviceBuffer, "upload", counting(E.DeviceBuffer.upload, lambda a, kw, r: np.asarray(a[1]).nbytes))
    monkeypatch.setattr(E.DeviceBuffer, "upload_at", counting(E.DeviceBuffer.upload_at, lambda a, kw, r: np.asarray(a[2]).nbytes))
    monkeypatch.setattr(E.DeviceBuffer, "download", counting(E.DeviceBuffer.download, lambda a, kw, r: r.nbytes))
    monkeypatch.setattr(E.DeviceBuffer, "download_at", counting(E.DeviceBuffer.download_at, lambda a, kw, r: r.nbytes))
    enc = co.sparsify(models, names)
    _e, le, bits, _t = enc.encoded[0]
    co.dynamic_masking()
    np.random.seed(3)
    up = co.quantize_encrypt(normalize=True)
    assert up.path == "sparse-cohort"
    out = {k: torch.empty_like(t) for k, t in models[0].items()}
    co.decrypt_unquantize(out=out, unnormalize=True)
    packed_bytes = 8 * ((le * bits + 63) // 64)
    uniforms = 8 * (le + 1) if le < DEVICE_RNG_MIN else 8
    budget = C * (packed_bytes + 2 * 4 * le + uniforms + 64 * 1024)
    assert moved[0] <= budget, (moved[0], budget)
