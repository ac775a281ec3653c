"""GPU: the sparse job's client step from a framework's device tensors -- Sparsifier over layers where they lie
(flashe_sparsify_tensors_dev), FlasheClient.quantize_encrypt of the compact layers it leaves in HBM plus the host 'zzz' layer, and
decrypt_unquantize(out=) of the dense aggregate -- byte for byte against the host path on the tensors' host copies (float16 / bfloat16:
`t.float().cpu().numpy()`), the reference's fixtures (sparsify.json, clientstep.json) and NumPy's stream position."""
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


def _host(t):
    """the host copy of INTEGRATION.md 2a"""
    import torch
    return (t.float() if t.dtype in (torch.float16, torch.bfloat16) else t).cpu().numpy()


def _tdt(torch, name):
    return {"float32": torch.float32, "float64": torch.float64, "float16": torch.float16, "bfloat16": torch.bfloat16}[name]


def _compact_bytes(v):
    from flashe_amd.weights import CompactLayer
    if isinstance(v, CompactLayer):
        return v.dtype, v.to_host().tobytes()
    a = np.asarray(v)
    return a.dtype, a.tobytes()


def _same_remain(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), k


# ---------------------------------------------------------------- 1. the reference's fixtures
def test_sparsify_golden_fed_as_tensors():
    torch = _torch()
    from flashe_amd import weights as wz
    for c in load_golden("sparsify.json")["cases"]:
        dt = np.dtype(c["dtype"])
        sp = wz.Sparsifier(c["sparsity"])
        for rd in c["rounds"]:
            layer = np.frombuffer(bytes.fromhex(rd["layer"]), dtype=dt).copy()
            t = torch.from_numpy(layer).cuda()
            w = {"w": t}
            enc, le, bits, total = sp.sparsify(w, ["w"])
            n = layer.size
            assert (le, bits, total) == (len(rd["location"]), n.bit_length(), n)
            assert (enc, le) == wz.to_big_int(np.array(rd["location"], dtype=np.uint64), bits)
            assert w["w"].to_host().tobytes().hex() == rd["masked"]
            r = sp.remain_weights["w"]
            assert r.dtype == dt and r.tobytes().hex() == rd["remain"]
            assert torch.equal(t, torch.from_numpy(layer).cuda())


# ---------------------------------------------------------------- 2. tensors against the host Sparsifier
SIZES = [1, 3, 1023, 1024, 1025, 4099, 70_001]


def _model(torch, dtypes, rnd, ties=True):
    g = torch.Generator(device="cpu").manual_seed(1000 + rnd)
    layers = {}
    for i, (n, dn) in enumerate(zip(SIZES, dtypes)):
        x = torch.randn(n, generator=g, dtype=torch.float64)
        layers[f"l{i}"] = x.to(_tdt(torch, dn)).cuda()
    if ties:
        # many equal bfloat16 magnitudes with either sign, a few larger ones; a constant layer; a view at an odd element offset
        x = torch.full((4099,), 0.5, dtype=torch.float64) * (torch.randint(0, 2, (4099,), generator=g) * 2 - 1)
        x[::37] = 3.0
        layers["tie"] = x.to(torch.bfloat16).cuda()
        layers["const"] = torch.full((1025,), 0.25, dtype=_tdt(torch, dtypes[0])).cuda()
        big = torch.randn(5000, generator=g, dtype=torch.float64).to(_tdt(torch, dtypes[-1])).cuda()
        layers["view"] = big[3:3 + 1025]
    return layers


@pytest.mark.parametrize("dtypes", [["float32"] * 7, ["float64"] * 7, ["float16"] * 7, ["bfloat16"] * 7,
                                    ["float32", "bfloat16", "float64", "float16", "float32", "float64", "bfloat16"]])
@pytest.mark.parametrize("sparsity", [0.1, 1e-7])
def test_tensors_against_the_host_sparsifier(dtypes, sparsity):
    torch = _torch()
    from flashe_amd.weights import CompactLayer, Sparsifier
    sp_t, sp_h = Sparsifier(sparsity), Sparsifier(sparsity)
    for rnd in range(3):
        layers = _model(torch, dtypes, rnd)
        before = {k: v.clone() for k, v in layers.items()}
        order = sorted(layers)
        wt = dict(layers)
        wh = {k: _host(v) for k, v in layers.items()}
        got = sp_t.sparsify(wt, order)
        want = sp_h.sparsify(wh, order)
        assert got == want, rnd
        for k in order:
            assert isinstance(wt[k], CompactLayer)
            assert _compact_bytes(wt[k]) == _compact_bytes(wh[k]), (rnd, k)
            assert torch.equal(layers[k], before[k]), k
        _same_remain(sp_t.remain_weights, sp_h.remain_weights)
        assert sp_t.shape_dict_used_for_sparsification == {k: tuple(v.shape) for k, v in layers.items()}


def test_host_tensor_host_rounds_continue_the_residuals():
    torch = _torch()
    from flashe_amd.weights import Sparsifier
    for dtypes in (["float32"] * 7, ["float32", "float64"] * 3 + ["bfloat16"]):
        sp_mix, sp_h = Sparsifier(0.05), Sparsifier(0.05)
        for rnd in range(3):
            layers = _model(torch, dtypes, 10 + rnd, ties=False)
            order = sorted(layers)
            wm = dict(layers) if rnd == 1 else {k: _host(v) for k, v in layers.items()}
            wh = {k: _host(v) for k, v in layers.items()}
            assert sp_mix.sparsify(wm, order) == sp_h.sparsify(wh, order)
            for k in order:
                assert _compact_bytes(wm[k]) == _compact_bytes(wh[k])
        _same_remain(sp_mix.remain_weights, sp_h.remain_weights)


# ---------------------------------------------------------------- 3. the reference's sparse client step with tensor compact layers
@pytest.mark.parametrize("case_i", [0, 1])
def test_clientstep_sparse_with_tensor_compact_layers(case_i):
    torch = _torch()
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheClient, aggregate_sparse_uploads
    from oracle.flashe_oracle import limbs_to_ints
    case = load_golden("clientstep.json")["sparse"][case_i]
    C = case["num_clients"]
    cm.N_JOBS = case["n_jobs"]
    cl0, uploads = None, []
    for c, rec in enumerate(case["clients"]):
        cl = FlasheClient({"quantize": {"int_bits": case["b"], "batch": False, "element_bits": case["element_bits"], "padding": True,
                                        "secure": True}, "precompute": {"enable": False}, "mask": "dynamic"})
        cl.create_cipher(c, C, KEY)
        cl.set_iter_index(case["iter"])
        cl.cipher.total = case["total"]
        cl.dynamic_masking(case["choice"], case["masks"])
        layers = {nm: torch.from_numpy(np.frombuffer(bytes.fromhex(rec["layers"][nm]), dtype=np.dtype(dt)).copy()).cuda()
                  for nm, _sh, dt in case["dense_layers"]}
        w = _W(layers)
        cl.quantizer.set_layer_size_list(w)
        w._weights["zzz"] = np.array([0.0])
        w.walking_order = sorted(w._weights, key=str)
        np.random.seed(rec["seed"])
        out = cl.quantize_encrypt(w, device=True)
        st = np.random.get_state()
        np.random.seed(rec["seed"])
        np.random.random(sum(int(v.numel()) for v in layers.values()) + 1)
        st_want = np.random.get_state()
        assert st[2] == st_want[2] and np.array_equal(st[1], st_want[1])
        k0 = rec["flat_key"]
        assert out.walking_order == [k0]
        v = out._weights[k0]
        assert len(v) == sum(int(t.numel()) for t in layers.values()) + 1
        assert limbs_to_ints(v.to_host()) == unhex(rec["upload"]), c
        uploads.append(v)
        cl0 = cl0 or cl
    agg = aggregate_sparse_uploads(cl0.cipher.engine, uploads, case["masks"], case["total"], device=True)
    assert limbs_to_ints(agg.to_host()) == unhex(case["agg"])
    cl0.set_idx_list(list(range(C)))
    cl0.shape_dict = {nm: tuple(sh) for nm, sh, _dt in case["dense_layers"]}
    outs = {nm: torch.empty(tuple(sh), dtype=torch.float64, device="cuda") for nm, sh, _dt in case["dense_layers"]}
    cl0.decrypt_unquantize(_W({case["clients"][0]["flat_key"]: agg}), out=outs)
    for nm, _sh, _dt in case["dense_layers"]:
        assert outs[nm].cpu().numpy().tobytes() == bytes.fromhex(case["unquantized"][nm]), nm


# ---------------------------------------------------------------- 4. / 5. the whole step, tensors against the host path
def _sizes(total):
    base = [9408, 4096, 16384, 36864, 65536, 147456, 262144, 589824, 1048576, 2359296, 2048000, 1000]
    out, at = [], 0
    for s in base * 20:
        if at + s > total:
            break
        out.append(s)
        at += s
    return out


def _step(torch, sizes, C, rounds, b, sparsity, tdtype, seed):
    """-> per round: (encoded tuples, uploads, aggregate, decrypted layers, mean / std lists, NumPy state) of the tensor path and the host
    path of C clients from the same values."""
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheClient, aggregate_sparse_uploads, dynamic_masking_choice
    from flashe_amd.engine import Engine
    from flashe_amd.weights import Sparsifier, from_big_int
    cm.N_JOBS = 16
    total = sum(sizes)
    names = [f"l{i:03d}" for i in range(len(sizes))]
    args = {"quantize": {"int_bits": b, "batch": False, "element_bits": 16, "padding": True, "secure": True}, "precompute": {"enable": False},
            "mask": "dynamic"}
    arb = Engine(KEY, b)
    paths = {}
    for path in ("tensor", "host"):
        cls, sps = [], []
        for c in range(C):
            cl = FlasheClient(args)
            cl.create_cipher(c, C, KEY)
            cl.cipher.total = total
            cls.append(cl)
            sps.append(Sparsifier(sparsity))
        res = []
        for rnd in range(rounds):
            g = torch.Generator(device="cpu").manual_seed(seed + rnd)
            encs, masks, compact = [], [], []
            for c in range(C):
                layers = {nm: (torch.randn(s, generator=g) * 0.05).to(tdtype).cuda() for nm, s in zip(names, sizes)}
                w = dict(layers) if path == "tensor" else {k: _host(v) for k, v in layers.items()}
                enc = sps[c].sparsify(w, names)
                encs.append(enc)
                masks.append(np.asarray(from_big_int(enc[0], enc[1], enc[2], as_object=False)).astype(np.int64))
                compact.append(w)
            choice = dynamic_masking_choice(masks, total)
            uploads = []
            for c, cl in enumerate(cls):
                cl.set_iter_index(rnd + 1)
                cl.dynamic_masking(choice, masks)
                w = _W(compact[c])
                w._weights["zzz"] = np.array([0.0])
                w.walking_order = sorted(w._weights, key=str)
                np.random.seed(seed * 100 + 10 * rnd + c)
                out = cl.quantize_encrypt(w, device=True, normalize=True)
                uploads.append(out._weights[out.walking_order[0]])
            state = np.random.get_state()
            agg = aggregate_sparse_uploads(arb, uploads, masks, total, device=True)
            cl = cls[0]
            if cl.cipher.masking_scheme != "single":
                res.append((encs, [u.to_host() for u in uploads], agg.to_host(), None, None, state))
                continue
            cl.set_idx_list(list(range(C)))
            cl.shape_dict = dict(sps[0].shape_dict_used_for_sparsification)
            if path == "tensor":
                outs = {nm: torch.empty(s, dtype=torch.float64, device="cuda") for nm, s in zip(names, sizes)}
                cl.decrypt_unquantize(_W({names[0]: agg}), out=outs, unnormalize=True)
                dec = {k: v.cpu().numpy() for k, v in outs.items()}
            else:
                back = cl.decrypt_unquantize(_W({names[0]: agg}), unnormalize=True)
                dec = {k: np.asarray(back._weights[k]) for k in names}
            stats = ([float(v).hex() for v in cl.quantizer.past_layer_mean_list], [float(v).hex() for v in cl.quantizer.past_layer_std_list])
            res.append((encs, [u.to_host() for u in uploads], agg.to_host(), dec, stats, state))
        paths[path] = res
    return paths


def _compare(paths):
    for rnd, (t, h) in enumerate(zip(paths["tensor"], paths["host"])):
        assert t[0] == h[0], rnd                                               # packed locations, le, bits, total
        assert all(np.array_equal(a, b) for a, b in zip(t[1], h[1])), rnd      # uploads
        assert np.array_equal(t[2], h[2]), rnd                                 # aggregate
        if t[3] is not None or h[3] is not None:
            assert t[3].keys() == h[3].keys()
            for k in t[3]:
                assert t[3][k].dtype == h[3][k].dtype and t[3][k].tobytes() == h[3][k].tobytes(), (rnd, k)
            assert t[4] == h[4], rnd
        assert t[5][2] == h[5][2] and np.array_equal(t[5][1], h[5][1]), rnd   # NumPy's state


@pytest.mark.parametrize("b,sparsity", [(20, 0.1), (128, 0.01)])
@pytest.mark.parametrize("tdtype", ["float32", "bfloat16"])
def test_ten_clients_three_rounds_tensor_step_against_host(b, sparsity, tdtype):
    torch = _torch()
    _compare(_step(torch, _sizes(2_100_000), 10, 3, b, sparsity, _tdt(torch, tdtype), 7))


def test_full_resnet50_size_client_against_host():
    torch = _torch()
    sizes = [9408] + [s for s in (4096, 16384, 36864, 65536, 147456, 262144, 589824, 1048576, 2359296) for _ in range(6)] + [2048000, 1000]
    _compare(_step(torch, sizes, 1, 1, 128, 0.01, torch.float32, 11))


# ---------------------------------------------------------------- 6. PCIe traffic
def test_no_dense_or_compact_layer_data_crosses_pcie(monkeypatch):
    torch = _torch()
    from flashe_amd import cipher as cm
    from flashe_amd import engine as E
    from flashe_amd.block import FlasheClient, aggregate_sparse_uploads
    from flashe_amd.quantize import DEVICE_RNG_MIN
    from flashe_amd.weights import Sparsifier, from_big_int
    cm.N_JOBS = 16
    sizes = {"a": 1_000_000, "b": 600_000, "c": 4099}
    total = sum(sizes.values())
    layers = {k: torch.randn(s, device="cuda") for k, s in sizes.items()}
    cl = FlasheClient({"quantize": {"int_bits": 128, "batch": False, "element_bits": 16, "padding": True, "secure": True},
                       "precompute": {"enable": False}, "mask": "dynamic"})
    cl.create_cipher(0, 1, KEY)
    cl.set_iter_index(1)
    cl.cipher.total = total
    sp = Sparsifier(0.01)
    sp.sparsify(dict(layers), sorted(sizes))                 # (first call: allocations, tables)
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
    # (Engine.upload goes through DeviceBuffer.upload: counted there once)
    w = dict(layers)
    enc, le, bits, _t = sp.sparsify(w, sorted(sizes))
    packed_bytes = 8 * ((le * bits + 63) // 64)
    client_side = moved[0]
    mask = np.asarray(from_big_int(enc, le, bits, as_object=False)).astype(np.int64)      # (what the arbiter sends back: not counted)
    moved[0] = client_side
    cl.dynamic_masking("single", [mask])
    ww = _W(w)
    ww._weights["zzz"] = np.array([0.0])
    ww.walking_order = sorted(ww._weights, key=str)
    np.random.seed(3)
    up = cl.quantize_encrypt(ww, device=True)
    client_side = moved[0]
    agg = aggregate_sparse_uploads(cl.cipher.engine, [up._weights["a"]], [mask], total, device=True)     # (the arbiter's pass: not counted)
    moved[0] = client_side
    cl.set_idx_list([0])
    cl.shape_dict = dict(sp.shape_dict_used_for_sparsification)
    out = {k: torch.empty_like(t) for k, t in layers.items()}
    cl.decrypt_unquantize(_W({"a": agg}), out=out, unnormalize=True)
    uniforms = 8 * (le + 1) if le < DEVICE_RNG_MIN else 8
    budget = packed_bytes + 2 * 4 * le + uniforms + 64 * 1024
    assert moved[0] <= budget, (moved[0], client_side, budget)


# ---------------------------------------------------------------- 7. stream order
def test_producer_on_a_side_stream_behind_a_long_kernel():
    torch = _torch()
    from flashe_amd.weights import Sparsifier
    n = 1 << 20
    vals = np.random.Generator(np.random.PCG64(5)).standard_normal(n).astype(np.float32)
    want_w = {"x": vals.copy()}
    want = Sparsifier(0.01).sparsify(want_w, ["x"])
    side = torch.cuda.Stream()
    x = torch.zeros(n, dtype=torch.float32, device="cuda")
    src = torch.from_numpy(vals).pin_memory()
    sp = Sparsifier(0.01)
    with torch.cuda.stream(side):
        torch.cuda._sleep(200_000_000)                                # bounded: well under a second
        x.copy_(src, non_blocking=True)
        w = {"x": x}
        got = sp.sparsify(w, ["x"])                                   # no host sync: the DLPack handshake orders it behind the copy
    assert got == want
    assert w["x"].to_host().tobytes() == want_w["x"].tobytes()


# ---------------------------------------------------------------- 8. refusals
def test_refusals_name_their_reason():
    torch = _torch()
    from flashe_amd.block import FlasheClient
    from flashe_amd.weights import Sparsifier
    sp = Sparsifier(0.1)
    good = torch.randn(100, device="cuda")
    for bad, what in [(torch.arange(100, device="cuda", dtype=torch.int32), "dtype"),
                      (torch.randn(10, 10, device="cuda").t(), "contiguous"),
                      (torch.randn(100, device="cuda", requires_grad=True), "grad")]:
        with pytest.raises((TypeError, ValueError, BufferError)) as ei:
            sp.sparsify({"a": good, "b": bad}, ["a", "b"])
        assert what in str(ei.value).lower(), str(ei.value)
    assert sp.remain_weights is None
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="device"):
            sp.sparsify({"a": good, "b": torch.randn(100, device="cuda:1")}, ["a", "b"])

    def client(batch=False, precompute=False):
        args = {"quantize": {"int_bits": 128, "batch": batch, "element_bits": 16, "padding": True, "secure": True},
                "precompute": {"enable": precompute, "num_params": 11}, "mask": "dynamic"}
        cl = FlasheClient(args)
        cl.create_cipher(0, 2, KEY)
        cl.set_iter_index(1)
        cl.cipher.total = 100
        return cl

    w = {"a": good}
    sp2 = Sparsifier(0.1)
    sp2.sparsify(w, ["a"])
    mask = list(range(10))

    def upload(cl):
        ww = _W({"a": w["a"]})
        ww._weights["zzz"] = np.array([0.0])
        ww.walking_order = ["a", "zzz"]
        return ww

    cl = client(batch=True)
    cl.dynamic_masking("single", [mask, mask])
    st = np.random.get_state()
    with pytest.raises(TypeError, match="batched"):
        cl.quantize_encrypt(upload(cl))
    assert np.array_equal(np.random.get_state()[1], st[1])
    cl = client(precompute=True)
    cl.dynamic_masking("single", [mask, mask])
    with pytest.raises(TypeError, match="precompute"):
        cl.quantize_encrypt(upload(cl))
    cl = client()
    cl.fuse = False
    with pytest.raises(TypeError, match="fuse"):
        cl.quantize_encrypt(upload(cl))
    # out= of the compact shape instead of the dense one
    cl = client()
    cl.dynamic_masking("single", [mask, mask])
    cl.quantize_encrypt(upload(cl), device=True)
    cl.set_idx_list([0, 1])
    cl.shape_dict = {"a": (100,)}
    from flashe_amd.engine import DeviceVector
    agg = DeviceVector.from_host(cl.cipher.engine, np.zeros((100, 2), dtype=np.uint64))
    with pytest.raises(ValueError, match="shape"):
        cl.decrypt_unquantize(_W({"a": agg}), out={"a": torch.empty(10, dtype=torch.float64, device="cuda")})
    assert "minus" in cl.cipher.next_iter_decrypt_prepared
    cl.cipher.masking_scheme = "double"
    with pytest.raises(TypeError, match="double"):
        cl.decrypt_unquantize(_W({"a": agg}), out={"a": torch.empty(100, dtype=torch.float64, device="cuda")})
