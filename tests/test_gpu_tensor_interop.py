"""GPU: framework device tensors through the cipher and the fused client step, bit for bit against the host path.

The yardstick of every case is the same call on the tensor's host copy (integers: np.asarray of it, int64 viewed as uint64; float16 /
bfloat16 layers: `t.float().cpu().numpy()`; results in a 32- or 16-bit `out`: `torch.from_numpy(host_f64).to(dtype)` on the CPU), with
the same NumPy RNG state.  Statistics are compared with ==, not a tolerance.  A torch-free producer (__cuda_array_interface__ over an
engine buffer) checks the interop without a framework."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEY = bytes(range(32))
IT = 6


class _W:
    def __init__(self, layers):
        self.walking_order = sorted(layers)
        self._weights = dict(layers)


def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible to torch")
    return torch


def _cipher(b, mask, idx, C=2, stream=None):
    from flashe_amd import FlasheCipher
    c = FlasheCipher(b, mask=mask, stream=stream)
    c.set_num_clients(C)
    c.generate_prp_seed(KEY)
    c.set_iter_index(IT)
    c.idx = idx
    return c


def _u64(x, n):
    """any result form (DeviceVector, uint32 / uint64 array, torch tensor) -> uint64 [n, k]"""
    from flashe_amd.engine import DeviceVector
    if isinstance(x, DeviceVector):
        x = x.to_host()
    elif not isinstance(x, np.ndarray):
        x = x.cpu().numpy()
    x = np.asarray(x)
    if x.dtype in (np.int64, np.int32):
        x = x.view(np.uint64 if x.dtype == np.int64 else np.uint32)
    return x.astype(np.uint64).reshape(n, -1)


# ---------------------------------------------------------------- integer operands
@pytest.mark.parametrize("b", [20, 64, 128])
@pytest.mark.parametrize("mask", ["single", "double"])
def test_integer_tensors_through_encrypt_aggregate_decrypt(b, mask):
    torch = _torch()
    from flashe_amd import cipher as cm
    cm.N_JOBS = 16
    n = 5003
    rng = np.random.Generator(np.random.PCG64(b))
    L = 2 if b > 64 else 1
    pts = [rng.integers(0, 2 ** min(b, 62), (n, L) if L == 2 else n, dtype=np.uint64) for _ in range(2)]
    if L == 2:
        for p in pts:
            p[:, 1] &= np.uint64((1 << (b - 64)) - 1)
    c0, c1 = _cipher(b, mask, 0), _cipher(b, mask, 1)
    tdts = [torch.uint64, torch.int64] + ([torch.int32] if b <= 32 else [])
    for tdt in tdts:
        def dev(a):
            if tdt == torch.int32:
                return torch.from_numpy(a.astype(np.uint32).view(np.int32)).cuda()
            return torch.from_numpy(a.view(np.int64)).cuda().to(tdt) if tdt == torch.uint64 else torch.from_numpy(a.view(np.int64)).cuda()
        host_pts = [p.astype(np.uint32) if tdt == torch.int32 else p for p in pts]
        want = [c.encrypt(hp) for c, hp in zip((c0, c1), host_pts)]
        got = [c.encrypt(dev(p)) for c, p in zip((c0, c1), pts)]
        for w, g in zip(want, got):
            assert np.array_equal(_u64(g, n), _u64(w, n)), (b, mask, tdt)
        o = torch.empty_like(dev(pts[0]))
        ptr = o.data_ptr()
        assert c0.encrypt(dev(pts[0]), out=o) is o and o.data_ptr() == ptr
        assert np.array_equal(_u64(o, n), _u64(want[0], n))
        # aggregate of the two ciphertexts handed as tensors, into a tensor
        ct_t = [torch.empty_like(o) for _ in range(2)]
        for c, p, t in zip((c0, c1), pts, ct_t):
            c.encrypt(dev(p), out=t)
        agg_w = c0.aggregate(want)
        agg_t = torch.empty_like(o)
        assert c0.aggregate(ct_t, out=agg_t) is agg_t
        assert np.array_equal(_u64(agg_t, n), _u64(agg_w, n))
        assert np.array_equal(_u64(c0.aggregate(ct_t), n), _u64(agg_w, n))
        c0.set_idx_list(raw_idx_list=[0, 1], mode="decrypt")
        dec_w = c0.decrypt(agg_w)
        c0.set_idx_list(raw_idx_list=[0, 1], mode="decrypt")
        dec_t = torch.empty_like(o)
        assert c0.decrypt(agg_t, out=dec_t) is dec_t
        assert np.array_equal(_u64(dec_t, n), _u64(dec_w, n))
        total = (pts[0].astype(object) + pts[1].astype(object)) if L == 1 else None
        if total is not None:
            assert [int(v) % (1 << b) for v in total[:50]] == [int(v) for v in _u64(dec_t, n)[:50, 0]]


class _CAI:
    """A torch-free producer: __cuda_array_interface__ v3 over an engine-allocated buffer."""

    def __init__(self, buf, n, typestr="<u8", readonly=False, offset=0):
        self.buf = buf
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (buf.ptr + offset, readonly), "version": 3, "strides": None,
                                         "stream": None}


def test_cuda_array_interface_producer_without_a_framework():
    from flashe_amd import cipher as cm
    cm.N_JOBS = 16
    n = 777
    c = _cipher(64, "double", 0)
    eng = c.engine
    pts = np.random.Generator(np.random.PCG64(3)).integers(0, 2 ** 62, n, dtype=np.uint64)
    src = eng.upload(pts)
    got = c.encrypt(_CAI(src, n))
    want = c.encrypt(pts)
    assert np.array_equal(_u64(got, n), _u64(want, n))
    dst = eng.alloc(8 * n)
    c.encrypt(_CAI(src, n), out=_CAI(dst, n))
    assert np.array_equal(dst.download(np.uint64, n), want)
    with pytest.raises(ValueError, match="read-only"):
        c.encrypt(_CAI(src, n), out=_CAI(dst, n, readonly=True))
    with pytest.raises(ValueError, match="aligned"):
        c.encrypt(_CAI(src, n - 1, offset=4))
    with pytest.raises(TypeError, match="unsupported dtype"):
        c.encrypt(_CAI(src, n, typestr="<f8"))


# ---------------------------------------------------------------- the client step
SHAPES = {"a_conv": ((16, 3, 5, 5), "float32"), "b_bias": ((16,), "float16"), "c_fc": ((300, 300), "bfloat16"), "d_dense": ((50, 7), "float64"),
          "e_out": ((70001,), "float32")}


def _client(b, C, idx, batch=False, eb=16, stream=None):
    from flashe_amd.block import FlasheClient
    args = {"quantize": {"int_bits": b, "batch": batch, "element_bits": eb, "padding": True, "secure": True}, "precompute": {"enable": False}}
    cl = FlasheClient(args, stream=stream)
    cl.create_cipher(idx, C, KEY)
    cl.set_iter_index(IT)
    return cl


def _layers(torch, seed, shapes=SHAPES, scale=0.05, shift=0.01):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return {k: (torch.randn(sh, generator=g, device="cuda", dtype=torch.float64) * scale + shift).to(getattr(torch, dt))
            for k, (sh, dt) in shapes.items()}


def _host(torch, layers):
    return {k: (t.float() if t.dtype in (torch.float16, torch.bfloat16) else t).cpu().numpy() for k, t in layers.items()}


def _set_stats(cl, n_layers, kind):
    q = cl.quantizer
    q.layer_size_list = [1] * n_layers
    if kind == "py":
        q.past_layer_mean_list = [0.003 * (i + 1) for i in range(n_layers)]
        q.past_layer_std_list = [0.04 + 0.01 * i for i in range(n_layers)]
    else:
        q.past_layer_mean_list = [np.float64(0.003) * (i + 1) for i in range(n_layers)]
        q.past_layer_std_list = [np.float64(0.04) + np.float64(0.01) * i for i in range(n_layers)]


@pytest.mark.parametrize("b,batch", [(20, False), (128, False), (128, True)])
@pytest.mark.parametrize("norm", [None, "py", "np"])
def test_quantize_encrypt_of_mixed_tensors_is_the_host_path(b, batch, norm):
    torch = _torch()
    from flashe_amd import cipher as cm
    cm.N_JOBS = 16
    C = 10
    layers = _layers(torch, 11)
    host = _host(torch, layers)
    ct, alphas = {}, {}
    for side in ("tensor", "host"):
        cl = _client(b, C, 3, batch=batch)
        if norm:
            _set_stats(cl, len(layers), norm)
        np.random.seed(42)
        w = _W(dict(layers) if side == "tensor" else {k: v.copy() for k, v in host.items()})
        out = cl.quantize_encrypt(w, device=True, normalize=bool(norm))
        ct[side] = out._weights[out.walking_order[0]].to_host()
        alphas[side] = list(cl.quantizer.alpha_list)
        assert np.random.get_state()[2] == ct.setdefault("pos", np.random.get_state()[2])
    assert alphas["tensor"] == alphas["host"]
    assert ct["tensor"].tobytes() == ct["host"].tobytes(), (b, batch, norm)


def _bits(torch, t):
    t = t.detach().cpu()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


@pytest.mark.parametrize("dt", ["float64", "float32", "float16", "bfloat16"])
@pytest.mark.parametrize("batch", [False, True])
def test_three_rounds_of_a_ten_client_step_into_model_tensors(dt, batch):
    """Three consecutive rounds, normalize + unnormalize, every client's model held as `dt` tensors on the device; the reference side is
    the host path with its layers cast to `dt` after every round.  Alphas, ciphertexts, values and statistics identical in every round."""
    torch = _torch()
    from flashe_amd import cipher as cm
    cm.N_JOBS = 16
    C, b = 10, 128
    tdt = getattr(torch, dt)
    shapes = {k: (sh, dt) for k, (sh, _d) in SHAPES.items()}
    shapes["d_dense"] = ((50, 7), "float64")                          # (one float64 layer in every model)
    model = _layers(torch, 5, shapes)
    cls_t = [_client(b, C, c, batch=batch) for c in range(C)]
    cls_h = [_client(b, C, c, batch=batch) for c in range(C)]
    for r in range(3):
        for cl in cls_t + cls_h:
            cl.set_iter_index(IT + r)
        cts_t, cts_h = [], []
        for c in range(C):
            g = torch.Generator(device="cuda").manual_seed(100 * r + c)
            upd = {k: (t.double() + 0.002 * torch.randn(t.shape, generator=g, device="cuda", dtype=torch.float64)).to(t.dtype)
                   for k, t in model.items()}
            host = _host(torch, upd)
            np.random.seed(1000 * r + c)
            wt = cls_t[c].quantize_encrypt(_W(upd), device=True, normalize=True)
            np.random.seed(1000 * r + c)
            wh = cls_h[c].quantize_encrypt(_W(host), device=True, normalize=True)
            assert cls_t[c].quantizer.alpha_list == cls_h[c].quantizer.alpha_list, (r, c)
            cts_t.append(wt._weights[wt.walking_order[0]])
            cts_h.append(wh._weights[wh.walking_order[0]])
            assert cts_t[-1].to_host().tobytes() == cts_h[-1].to_host().tobytes(), (r, c)
        agg = cls_t[0].cipher.aggregate(cts_t)
        first = sorted(model)[0]
        new_model = None
        for c in range(C):
            cls_t[c].set_idx_list(list(range(C)))
            cls_h[c].set_idx_list(list(range(C)))
            out = {k: torch.empty_like(t) for k, t in model.items()}
            res = cls_t[c].decrypt_unquantize(_W({first: agg}), out=out, unnormalize=True)
            assert all(res._weights[k] is out[k] for k in out)
            want = cls_h[c].decrypt_unquantize(_W({first: agg}), unnormalize=True)
            for k in model:
                ref = torch.from_numpy(np.ascontiguousarray(want._weights[k])).to(out[k].dtype)
                assert torch.equal(_bits(torch, out[k]), _bits(torch, ref)), (r, c, k)
            qt, qh = cls_t[c].quantizer, cls_h[c].quantizer
            assert [type(v) for v in qt.past_layer_mean_list] == [np.float64] * len(model)
            assert qt.past_layer_mean_list == qh.past_layer_mean_list, (r, c)
            assert qt.past_layer_std_list == qh.past_layer_std_list, (r, c)
            if c == 0:
                new_model = out
        model = new_model


@pytest.mark.parametrize("dt", ["float64", "float32", "float16", "bfloat16"])
def test_decrypt_unquantize_into_out_without_unnormalize(dt):
    torch = _torch()
    from flashe_amd import cipher as cm
    cm.N_JOBS = 16
    C = 2
    layers = _layers(torch, 9)
    cls = [_client(20, C, c) for c in range(C)]
    cts = []
    for c, cl in enumerate(cls):
        np.random.seed(c)
        w = cl.quantize_encrypt(_W(dict(layers)), device=True)
        cts.append(w._weights[w.walking_order[0]])
    agg = cls[0].cipher.aggregate(cts)
    first = sorted(layers)[0]
    cls[0].set_idx_list([0, 1])
    want = cls[0].decrypt_unquantize(_W({first: agg}))
    cls[0].set_idx_list([0, 1])
    out = {k: torch.empty(t.shape, dtype=getattr(torch, dt), device="cuda") for k, t in layers.items()}
    means = list(cls[0].quantizer.past_layer_mean_list)
    cls[0].decrypt_unquantize(_W({first: agg}), out=out)
    assert cls[0].quantizer.past_layer_mean_list == means
    for k in layers:
        ref = torch.from_numpy(np.ascontiguousarray(want._weights[k])).to(getattr(torch, dt))
        assert torch.equal(_bits(torch, out[k]), _bits(torch, ref)), k


def test_full_size_f32_client_step_against_the_host_path():
    torch = _torch()
    from flashe_amd import cipher as cm
    cm.N_JOBS = 16
    sizes = [9408] + [s for s in (4096, 16384, 36864, 65536, 147456, 262144, 589824, 1048576, 2359296) for _ in range(6)] + [2048000, 1000]
    g = torch.Generator(device="cuda").manual_seed(0)
    layers = {f"l{i:03d}": torch.randn(s, generator=g, device="cuda", dtype=torch.float32) * 0.05 for i, s in enumerate(sizes)}
    host = _host(torch, layers)
    res = {}
    for side, w in (("tensor", dict(layers)), ("host", host)):
        cl = _client(128, 10, 3)
        np.random.seed(8)
        out = cl.quantize_encrypt(_W(w), device=True)
        res[side] = out._weights[out.walking_order[0]].to_host()
    assert res["tensor"].tobytes() == res["host"].tobytes()


def test_no_layer_data_crosses_pcie(monkeypatch):
    torch = _torch()
    from flashe_amd import cipher as cm
    from flashe_amd import engine as E
    cm.N_JOBS = 16
    moved = [0]

    def counting(fn, size_of):
        def wrap(*a, **kw):
            r = fn(*a, **kw)
            moved[0] += size_of(a, kw, r)
            return r
        return wrap

    layers = _layers(torch, 3, {"a": ((1000, 1000), "float32"), "b": ((48,), "bfloat16")})
    cl = _client(128, 1, 0)
    first = "a"
    monkeypatch.setattr(E.Engine, "upload", counting(E.Engine.upload, lambda a, kw, r: np.asarray(a[1]).nbytes))
    monkeypatch.setattr(E.DeviceBuffer, "upload", counting(E.DeviceBuffer.upload, lambda a, kw, r: np.asarray(a[1]).nbytes))
    monkeypatch.setattr(E.DeviceBuffer, "upload_at", counting(E.DeviceBuffer.upload_at, lambda a, kw, r: np.asarray(a[2]).nbytes))
    monkeypatch.setattr(E.DeviceBuffer, "download", counting(E.DeviceBuffer.download, lambda a, kw, r: r.nbytes))
    monkeypatch.setattr(E.DeviceBuffer, "download_at", counting(E.DeviceBuffer.download_at, lambda a, kw, r: r.nbytes))
    np.random.seed(1)
    w = cl.quantize_encrypt(_W(layers), device=True)
    assert moved[0] < 64 * 1024, moved[0]
    cl.set_idx_list([0])
    out = {k: torch.empty_like(t) for k, t in layers.items()}
    cl.decrypt_unquantize(_W({first: w._weights[first]}), out=out, unnormalize=True)
    assert moved[0] < 64 * 1024, moved[0]


# ---------------------------------------------------------------- stream order and lifetime
def test_producer_on_a_side_stream_behind_a_long_kernel():
    torch = _torch()
    from flashe_amd import cipher as cm
    cm.N_JOBS = 16
    n = 1 << 20
    pts = np.random.Generator(np.random.PCG64(5)).integers(0, 2 ** 62, n, dtype=np.uint64)
    c = _cipher(64, "double", 0)
    want = c.encrypt(pts)
    side = torch.cuda.Stream()
    x = torch.zeros(n, dtype=torch.int64, device="cuda")
    src = torch.from_numpy(pts.view(np.int64)).pin_memory()
    with torch.cuda.stream(side):
        torch.cuda._sleep(200_000_000)                                # bounded: well under a second
        x.copy_(src, non_blocking=True)
        got = c.encrypt(x)                                            # no host sync: the DLPack handshake orders it behind the copy
    assert np.array_equal(_u64(got, n), _u64(want, n))


def test_a_dropped_plaintext_is_not_reused_while_the_encrypt_reads_it():
    torch = _torch()
    from flashe_amd import cipher as cm
    cm.N_JOBS = 16
    n = 1 << 22
    pts = np.random.Generator(np.random.PCG64(6)).integers(0, 2 ** 62, n, dtype=np.uint64)
    c = _cipher(128, "double", 0)
    want = c.encrypt(pts)
    x = torch.from_numpy(pts.view(np.int64)).cuda()
    torch.cuda.synchronize()
    got = c.encrypt(x)
    del x
    y = torch.full((n,), 7, dtype=torch.int64, device="cuda")        # allocated and filled at once, on the framework's stream
    assert np.array_equal(_u64(got, n), _u64(want, n))
    assert int(y[0]) == 7


def test_consumer_reads_out_on_the_framework_stream_in_shared_stream_mode():
    torch = _torch()
    from flashe_amd import cipher as cm
    cm.N_JOBS = 16
    layers = _layers(torch, 21, {"a": ((400, 300), "float32"), "b": ((300,), "float32")})
    stream = torch.cuda.current_stream().cuda_stream
    cl = _client(128, 1, 0, stream=stream)
    ref = _client(128, 1, 0)
    np.random.seed(4)
    w = cl.quantize_encrypt(_W(dict(layers)), device=True)
    np.random.seed(4)
    wr = ref.quantize_encrypt(_W(_host(torch, layers)), device=True)
    cl.set_idx_list([0])
    ref.set_idx_list([0])
    out = {k: torch.empty_like(t) for k, t in layers.items()}
    cl.decrypt_unquantize(_W({"a": w._weights["a"]}), out=out)
    sums = {k: out[k].double().sum() for k in out}                   # queued right behind the store, no sync in between
    want = ref.decrypt_unquantize(_W({"a": wr._weights["a"]}))
    for k in out:
        assert float(sums[k]) == float(torch.from_numpy(want._weights[k]).float().double().sum())


# ---------------------------------------------------------------- refusals
def test_refusals_name_their_reason():
    torch = _torch()
    from flashe_amd import cipher as cm
    cm.N_JOBS = 16
    c = _cipher(64, "double", 0)
    x = torch.arange(64, dtype=torch.int64, device="cuda").reshape(8, 8)
    with pytest.raises(ValueError, match="C-contiguous"):
        c.encrypt(x.T)
    with pytest.raises(TypeError, match="unsupported dtype"):
        c.encrypt(torch.zeros(8, dtype=torch.float32, device="cuda"))
    with pytest.raises(TypeError, match="out: unsupported dtype"):
        c.encrypt(torch.zeros(8, dtype=torch.int64, device="cuda"), out=torch.zeros(8, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="out: expected shape"):
        c.encrypt(torch.zeros(8, dtype=torch.int64, device="cuda"), out=torch.zeros(9, dtype=torch.int64, device="cuda"))
    with pytest.raises(TypeError, match="packed"):
        c.aggregate([torch.zeros(8, dtype=torch.int64, device="cuda")], packed=True, out=torch.zeros(8, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="ROCm device memory"):
        c.encrypt(torch.zeros(8, dtype=torch.int64))
    cl = _client(128, 1, 0)
    layers = {"a": torch.zeros(100, device="cuda", requires_grad=True)}
    with pytest.raises(BufferError, match="require gradient"):
        cl.quantize_encrypt(_W(layers))
    np.random.seed(0)
    w = cl.quantize_encrypt(_W({"a": torch.zeros(100, device="cuda")}))
    cl.set_idx_list([0])
    with pytest.raises(ValueError, match="expected shape"):
        cl.decrypt_unquantize(_W({"a": w._weights["a"]}), out={"a": torch.zeros(99, device="cuda")})
    with pytest.raises(TypeError, match="unsupported dtype"):
        cl.decrypt_unquantize(_W({"a": w._weights["a"]}), out={"a": torch.zeros(100, dtype=torch.int32, device="cuda")})


def test_a_tensor_on_another_device_is_refused():
    torch = _torch()
    if torch.cuda.device_count() < 2:
        pytest.skip("a second device is needed for the wrong-device refusal")
    c = _cipher(64, "double", 0)
    with pytest.raises(ValueError, match="device 1, this engine on device 0"):
        c.encrypt(torch.zeros(8, dtype=torch.int64, device="cuda:1"))
