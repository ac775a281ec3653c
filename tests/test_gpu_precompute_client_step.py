"""GPU: the fused client step of precompute jobs -- the masks prepare_encrypt / prepare_decrypt leave in the engine's ctx added by the
codec launches in place of the PRF streams -- from host layers and from framework tensors, against the reference's jobs
(tests/golden/clientstep.json) and bit for bit against the call-by-call step (which clientstep.json and block.json pin to the reference):
ciphertexts, floats, NumPy's stream position and the state of next_iter_encrypt_prepared / next_iter_decrypt_prepared(_idx)."""
import numpy as np
import pytest

from conftest import load_golden, unhex

pytestmark = pytest.mark.gpu

KEY = bytes(range(32))
IT = 6

try:
    # (asked at collection: once a test has created an engine, the framework of the same process no longer finds its device)
    import torch as _torch_mod
    _TORCH_GPU = _torch_mod.cuda.is_available()
except ImportError:
    _TORCH_GPU = False


class _W:
    def __init__(self, layers):
        self.walking_order = sorted(layers)
        self._weights = dict(layers)


def _torch():
    torch = pytest.importorskip("torch")
    if not (_TORCH_GPU and torch.cuda.is_available()):
        pytest.skip("no GPU visible to torch")
    return torch


def _client(b, C, idx, num_params, batch=False, eb=16, fuse=True, scheme="double"):
    """A precompute client at iteration IT whose encrypt masks were prepared in the job's order: at IT - 1, for IT."""
    from flashe_amd.block import FlasheClient
    args = {"quantize": {"int_bits": b, "batch": batch, "element_bits": eb, "padding": True, "secure": True},
            "precompute": {"enable": True, "num_params": num_params}}
    cl = FlasheClient(args)
    cl.create_cipher(idx, C, KEY)
    cl.cipher.masking_scheme = scheme
    cl.fuse = fuse
    cl.set_iter_index(IT - 1)
    cl.prepare_encrypt()
    cl.set_iter_index(IT)
    return cl


def _n_ct(sizes, b, batch, C, eb=16):
    if not batch:
        return sum(sizes)
    bs = b // (eb + int(np.ceil(np.log2(C))))
    return sum((s + bs - 1) // bs for s in sizes)


def _limbs(v, L):
    """a ciphertext in any form the step returns (DeviceVector, uint64 limbs, object ints) -> uint64 [n, L]"""
    from flashe_amd.cipher import _to_limbs
    from flashe_amd.engine import DeviceVector
    if isinstance(v, DeviceVector):
        v = v.to_host()
    v = np.asarray(v)
    return v.reshape(v.shape[0], -1) if v.dtype == np.uint64 else _to_limbs(v, L)[0]


def _rng_pos():
    st = np.random.get_state()
    return st[2], st[1].copy()


def _same_pos(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1])


# ---------------------------------------------------------------- 1. the reference jobs with precompute
@pytest.mark.parametrize("case_i", range(8))
def test_precompute_jobs_are_the_reference_jobs(case_i):
    """Every dense case of clientstep.json run as a precompute job: quantize_encrypt(device=True) returns a DeviceVector equal to the
    fixture's ciphertext, consumes NumPy's stream one draw per value and the encrypt cache (a single-mask cipher drops only 'add', as the
    reference does); after prepare_decrypt and set_idx_list(all), decrypt_unquantize of both aggregates gives the fixture's floats byte for
    byte -- with the next round's encrypt cache present (the job prepares it while it waits for the aggregate), which the decrypt leaves."""
    from flashe_amd import cipher as cm
    from flashe_amd.engine import DeviceVector
    from oracle.flashe_oracle import limbs_to_ints
    case = load_golden("clientstep.json")["dense"][case_i]
    b, C, it = case["b"], case["num_clients"], case["iter"]
    cm.N_JOBS = case["n_jobs"]
    n_values = sum(int(np.prod(sh)) for _nm, sh, _dt in case["layers"])
    n_ct = len(case["clients"][0]["flat_ct"])
    from flashe_amd.block import FlasheClient
    args = {"quantize": {"int_bits": b, "batch": bool(case.get("batch")), "element_bits": case["element_bits"], "padding": True, "secure": True},
            "precompute": {"enable": True, "num_params": n_ct}}
    clients, cts = [], []
    for c, rec in enumerate(case["clients"]):
        cl = FlasheClient(args)
        cl.create_cipher(c, C, KEY)
        cl.cipher.masking_scheme = case["scheme"]
        if it > 0:
            cl.set_iter_index(it - 1)
            cl.prepare_encrypt()
        cl.set_iter_index(it)
        layers = {nm: np.frombuffer(bytes.fromhex(rec["layers"][nm]), dtype=np.dtype(dt)).copy().reshape(sh) for nm, sh, dt in case["layers"]}
        np.random.seed(rec["seed"])
        out = cl.quantize_encrypt(_W(layers), device=True)
        got_pos = _rng_pos()
        np.random.seed(rec["seed"])
        np.random.random(n_values)
        assert _same_pos(got_pos, _rng_pos()), "the NumPy stream must be consumed as the reference consumes it"
        v = out._weights[rec["flat_key"]]
        assert isinstance(v, DeviceVector)
        assert limbs_to_ints(v.to_host()) == unhex(rec["flat_ct"]), (case_i, c)
        assert set(cl.cipher.next_iter_encrypt_prepared) == (set() if case["scheme"] == "double" else {"minus"})
        held = cl.cipher.engine.prepared_query(cl.cipher.engine.PREPARED_ENCRYPT)[0]
        assert held == (case["scheme"] != "double"), "the fused double-mask step consumes the ctx's cache"
        clients.append(cl)
        cts.append(v)
    agg_elem = clients[0].cipher.aggregate(cts)
    agg_packed = clients[0].cipher.aggregate(cts, packed=True)
    cl = clients[0]
    for agg, out_name in ((agg_elem, "out_elem"), (agg_packed, "out_packed")):
        cl.prepare_encrypt()
        cl.prepare_decrypt()
        cl.set_idx_list(list(range(C)))
        back = cl.decrypt_unquantize(_W({case["clients"][0]["flat_key"]: agg}))
        for nm, sh, _dt in case["layers"]:
            assert np.asarray(back._weights[nm], dtype=np.float64).tobytes() == bytes.fromhex(case[out_name]["unquantized"][nm]), (case_i, out_name, nm)
        if case["scheme"] == "double":
            assert cl.cipher.next_iter_decrypt_prepared == {} and cl.cipher.next_iter_decrypt_prepared_idx == {}
        else:
            assert set(cl.cipher.next_iter_decrypt_prepared) == {"add"}
        assert set(cl.cipher.next_iter_encrypt_prepared) == {"add", "minus"}
        assert cl.cipher.engine.prepared_query(cl.cipher.engine.PREPARED_ENCRYPT)[0], "the decrypt must leave the encrypt cache alone"


# ---------------------------------------------------------------- 2. ten clients, three rounds, tensors
SHAPES = {"a_conv": (16, 3, 5, 5), "b_bias": (16,), "c_fc": (300, 300), "d_dense": (50, 7), "e_out": (70001,)}


def _host(torch, layers):
    return {k: (t.float() if t.dtype in (torch.float16, torch.bfloat16) else t).cpu().numpy() for k, t in layers.items()}


def _bits(torch, t):
    t = t.detach().cpu()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


@pytest.mark.parametrize("dt", ["float32", "float64", "float16", "bfloat16"])
@pytest.mark.parametrize("b,batch", [(20, False), (120, True)])
def test_three_precompute_rounds_of_ten_clients_from_tensors(dt, b, batch):
    """The job's order over three rounds: the encrypt masks of a round prepared at the end of the previous one (after the upload), the
    decrypt masks after the upload too; normalize + unnormalize; client 1 drops out of the second round (the decrypt's extra prefixes; its
    stale encrypt cache is used in the third round, as the reference uses it).  The tensor side (layers `dt` on the device, out= tensors)
    against the call-by-call step on the host copies: alphas, ciphertexts, values and statistics identical (==) in every round."""
    torch = _torch()
    from flashe_amd import cipher as cm
    cm.N_JOBS = 16
    C = 10
    tdt = getattr(torch, dt)
    g = torch.Generator(device="cuda").manual_seed(5)
    model = {k: (torch.randn(sh, generator=g, device="cuda", dtype=torch.float64) * 0.05 + 0.01).to(torch.float64 if k == "d_dense" else tdt)
             for k, sh in SHAPES.items()}
    n_ct = _n_ct([int(np.prod(sh)) for sh in SHAPES.values()], b, batch, C)
    L = 2 if b > 64 else 1
    cls_t = [_client(b, C, c, n_ct, batch=batch) for c in range(C)]
    cls_h = [_client(b, C, c, n_ct, batch=batch, fuse=False) for c in range(C)]
    first = sorted(model)[0]
    for r in range(3):
        up = [c for c in range(C) if not (r == 1 and c == 1)]
        for c in up:
            cls_t[c].set_iter_index(IT + r)
            cls_h[c].set_iter_index(IT + r)
        cts_t = []
        for c in up:
            gc = torch.Generator(device="cuda").manual_seed(100 * r + c)
            upd = {k: (t.double() + 0.002 * torch.randn(t.shape, generator=gc, device="cuda", dtype=torch.float64)).to(t.dtype) for k, t in model.items()}
            host = _host(torch, upd)
            np.random.seed(1000 * r + c)
            wt = cls_t[c].quantize_encrypt(_W(upd), device=True, normalize=True)
            pos_t = _rng_pos()
            np.random.seed(1000 * r + c)
            wh = cls_h[c].quantize_encrypt(_W(host), normalize=True)
            assert _same_pos(pos_t, _rng_pos())
            assert cls_t[c].quantizer.alpha_list == cls_h[c].quantizer.alpha_list, (r, c)
            ct_t = wt._weights[wt.walking_order[0]]
            assert np.array_equal(_limbs(ct_t, L), _limbs(wh._weights[wh.walking_order[0]], L)), (r, c)
            assert cls_t[c].cipher.next_iter_encrypt_prepared == cls_h[c].cipher.next_iter_encrypt_prepared == {}
            cts_t.append(ct_t)
        agg = cls_t[up[0]].cipher.aggregate(cts_t)
        new_model = None
        for c in up:
            for cl in (cls_t[c], cls_h[c]):
                cl.prepare_encrypt()                              # the next round's masks, while the arbiter aggregates
                cl.prepare_decrypt()
                cl.set_idx_list(list(up))
            out = {k: torch.empty_like(t) for k, t in model.items()}
            res = cls_t[c].decrypt_unquantize(_W({first: agg}), out=out, unnormalize=True)
            assert all(res._weights[k] is out[k] for k in out)
            want = cls_h[c].decrypt_unquantize(_W({first: agg}), unnormalize=True)
            for k in model:
                ref = torch.from_numpy(np.ascontiguousarray(want._weights[k])).to(out[k].dtype)
                assert torch.equal(_bits(torch, out[k]), _bits(torch, ref)), (r, c, k)
            qt, qh = cls_t[c].quantizer, cls_h[c].quantizer
            assert qt.past_layer_mean_list == qh.past_layer_mean_list and qt.past_layer_std_list == qh.past_layer_std_list, (r, c)
            for side in (cls_t[c], cls_h[c]):
                assert side.cipher.next_iter_decrypt_prepared == {} and side.cipher.next_iter_decrypt_prepared_idx == {}
                assert set(side.cipher.next_iter_encrypt_prepared) == {"add", "minus"}
            if c == 0:
                new_model = out
        model = new_model


# ---------------------------------------------------------------- 3. PCIe bytes
def test_precompute_step_from_tensors_moves_no_layer_over_pcie(monkeypatch):
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

    g = torch.Generator(device="cuda").manual_seed(3)
    layers = {"a": torch.randn((1000, 1000), generator=g, device="cuda") * 0.05, "b": (torch.randn(48, generator=g, device="cuda") * 0.05).to(torch.bfloat16)}
    for b, batch in ((20, False), (120, True)):
        cl = _client(b, 2, 0, _n_ct([1000 * 1000, 48], b, batch, 2), batch=batch)
        cl.prepare_decrypt()
        moved[0] = 0
        with monkeypatch.context() as m:
            m.setattr(E.Engine, "upload", counting(E.Engine.upload, lambda a, kw, r: np.asarray(a[1]).nbytes))
            m.setattr(E.DeviceBuffer, "upload", counting(E.DeviceBuffer.upload, lambda a, kw, r: np.asarray(a[1]).nbytes))
            m.setattr(E.DeviceBuffer, "upload_at", counting(E.DeviceBuffer.upload_at, lambda a, kw, r: np.asarray(a[2]).nbytes))
            m.setattr(E.DeviceBuffer, "download", counting(E.DeviceBuffer.download, lambda a, kw, r: r.nbytes))
            m.setattr(E.DeviceBuffer, "download_at", counting(E.DeviceBuffer.download_at, lambda a, kw, r: r.nbytes))
            np.random.seed(1)
            w = cl.quantize_encrypt(_W(layers), device=True)
            assert cl.cipher.next_iter_encrypt_prepared == {}
            cl.set_idx_list([0, 1])
            out = {k: torch.empty_like(t) for k, t in layers.items()}
            cl.decrypt_unquantize(_W({"a": w._weights["a"]}), out=out, unnormalize=True)
            assert cl.cipher.next_iter_decrypt_prepared == {}
        assert moved[0] < 64 * 1024, (b, moved[0])


# ---------------------------------------------------------------- 4. the cache state machine
def _layers_host(seed, sizes=(3000, 17, 5000)):
    rng = np.random.Generator(np.random.PCG64(seed))
    return {f"l{i}": (rng.standard_normal(s) * 0.05).astype(np.float32) for i, s in enumerate(sizes)}


@pytest.mark.parametrize("b,batch", [(20, False), (128, False), (120, True)])
def test_a_length_mismatch_keeps_the_cache_and_the_stream_position(b, batch):
    from flashe_amd import cipher as cm
    cm.N_JOBS = 16
    n_ct = _n_ct([3000, 17, 5000], b, batch, 4)
    pos, msgs = {}, {}
    for fuse in (True, False):
        cl = _client(b, 4, 1, n_ct + 1, batch=batch, fuse=fuse)
        np.random.seed(7)
        with pytest.raises(ValueError) as e:
            cl.quantize_encrypt(_W(_layers_host(0)), device=True)
        pos[fuse], msgs[fuse] = _rng_pos(), str(e.value)
        assert set(cl.cipher.next_iter_encrypt_prepared) == {"add", "minus"}
        assert cl.cipher.engine.prepared_query(cl.cipher.engine.PREPARED_ENCRYPT)[:2] == (True, n_ct + 1)
    assert _same_pos(pos[True], pos[False]) and msgs[True] == msgs[False]


@pytest.mark.parametrize("b,batch", [(20, False), (120, True)])
def test_a_second_encrypt_without_a_prepare_is_the_online_fused_step(b, batch):
    from flashe_amd import cipher as cm
    from flashe_amd.engine import DeviceVector
    cm.N_JOBS = 16
    L = 2 if b > 64 else 1
    n_ct = _n_ct([3000, 17, 5000], b, batch, 4)
    pre = _client(b, 4, 2, n_ct, batch=batch)
    ref = _client(b, 4, 2, n_ct, batch=batch)
    ref.cipher.next_iter_encrypt_prepared = {}                    # (a caller dropping the cache: the ctx discards it)
    np.random.seed(3)
    pre.quantize_encrypt(_W(_layers_host(1)), device=True)
    assert pre.cipher.next_iter_encrypt_prepared == {}
    np.random.seed(4)
    got = pre.quantize_encrypt(_W(_layers_host(2)), device=True)
    np.random.seed(4)
    want = ref.quantize_encrypt(_W(_layers_host(2)), device=True)
    assert not ref.cipher.engine.prepared_query(ref.cipher.engine.PREPARED_ENCRYPT)[0]
    g, w = got._weights["l0"], want._weights["l0"]
    assert isinstance(g, DeviceVector) and np.array_equal(_limbs(g, L), _limbs(w, L))


@pytest.mark.parametrize("b,batch", [(20, False), (128, False), (120, True)])
def test_a_single_mask_cipher_with_caches_is_the_call_by_call_step(b, batch):
    from flashe_amd import cipher as cm
    cm.N_JOBS = 16
    L = 2 if b > 64 else 1
    n_ct = _n_ct([3000, 17, 5000], b, batch, 4)
    res = {}
    for fuse in (True, False):
        cls = [_client(b, 4, c, n_ct, batch=batch, fuse=fuse, scheme="single") for c in range(4)]
        cts = []
        for c, cl in enumerate(cls):
            np.random.seed(10 + c)
            w = cl.quantize_encrypt(_W(_layers_host(c)), device=True)
            cts.append(_limbs(w._weights["l0"], L))
        enc_dicts = [sorted(cl.cipher.next_iter_encrypt_prepared) for cl in cls]
        agg = cls[0].cipher.aggregate([np.ascontiguousarray(a) for a in cts])
        cls[0].prepare_decrypt()
        cls[0].set_idx_list(list(range(4)))
        back = cls[0].decrypt_unquantize(_W({"l0": agg}))
        res[fuse] = (cts, enc_dicts, sorted(cls[0].cipher.next_iter_decrypt_prepared), sorted(cls[0].cipher.next_iter_decrypt_prepared_idx),
                     {k: np.asarray(v, dtype=np.float64).tobytes() for k, v in back._weights.items()})
    got, want = res[True], res[False]
    assert all(np.array_equal(x, y) for x, y in zip(got[0], want[0]))
    assert got[1:] == want[1:]
    assert got[1] == [["minus"]] * 4


@pytest.mark.parametrize("b,batch", [(20, False), (120, True)])
def test_a_decrypt_leaves_the_next_rounds_encrypt_cache(b, batch):
    """Both caches present (the job prepares them together): the fused decrypt consumes the decrypt cache only; the next round's
    encrypt then consumes the encrypt cache and equals the call-by-call step."""
    from flashe_amd import cipher as cm
    cm.N_JOBS = 16
    L = 2 if b > 64 else 1
    n_ct = _n_ct([3000, 17, 5000], b, batch, 2)
    sides = {}
    for fuse in (True, False):
        cls = [_client(b, 2, c, n_ct, batch=batch, fuse=fuse) for c in range(2)]
        cts = []
        for c, cl in enumerate(cls):
            np.random.seed(20 + c)
            cts.append(cl.quantize_encrypt(_W(_layers_host(c)), device=True)._weights["l0"])
        agg = cls[0].cipher.aggregate([np.ascontiguousarray(_limbs(x, L)) for x in cts])
        cl = cls[0]
        cl.prepare_encrypt()
        cl.prepare_decrypt()
        cl.set_idx_list([0, 1])
        back = cl.decrypt_unquantize(_W({"l0": agg}))
        eng = cl.cipher.engine
        assert set(cl.cipher.next_iter_encrypt_prepared) == {"add", "minus"} and eng.prepared_query(eng.PREPARED_ENCRYPT)[0]
        assert cl.cipher.next_iter_decrypt_prepared == {} and not eng.prepared_query(eng.PREPARED_DECRYPT)[0]
        cl.set_iter_index(IT + 1)
        np.random.seed(30)
        nxt = cl.quantize_encrypt(_W(_layers_host(5)), device=True)._weights["l0"]
        assert cl.cipher.next_iter_encrypt_prepared == {}
        sides[fuse] = ({k: np.asarray(v, dtype=np.float64).tobytes() for k, v in back._weights.items()}, _limbs(nxt, L))
    assert sides[True][0] == sides[False][0]
    assert np.array_equal(sides[True][1], sides[False][1])


# ---------------------------------------------------------------- 5. integer tensors through the cipher
@pytest.mark.parametrize("b", [20, 64, 128])
def test_integer_tensors_through_the_cipher_with_prepared_masks(b):
    torch = _torch()
    from flashe_amd import FlasheCipher
    from flashe_amd import cipher as cm
    cm.N_JOBS = 16
    n = 5003
    L = 2 if b > 64 else 1
    rng = np.random.Generator(np.random.PCG64(b))
    pt = rng.integers(0, 2 ** min(b, 62), (n, L) if L == 2 else n, dtype=np.uint64)
    if L == 2:
        pt[:, 1] &= np.uint64((1 << (b - 64)) - 1)

    def cipher():
        c = FlasheCipher(b)
        c.set_num_clients(3)
        c.generate_prp_seed(KEY)
        c.idx = 1
        c.set_num_params(n)
        c.set_iter_index(IT - 1)
        c.prepare_encrypt()
        c.set_iter_index(IT)
        return c

    tdts = [torch.int64] + ([torch.int32] if b <= 32 else [])
    for tdt in tdts:
        signed, unsigned = (np.int32, np.uint32) if tdt == torch.int32 else (np.int64, np.uint64)
        ct_, ch = cipher(), cipher()
        host = pt.astype(unsigned)
        got = ct_.encrypt(torch.from_numpy(host.view(signed)).cuda())
        want = ch.encrypt(host)
        assert np.array_equal(got.to_host().astype(np.uint64).reshape(n, -1), want.astype(np.uint64).reshape(n, -1)), (b, tdt)
        assert ct_.next_iter_encrypt_prepared == ch.next_iter_encrypt_prepared == {}
        for c in (ct_, ch):
            c.prepare_decrypt()
            c.set_idx_list(raw_idx_list=[0, 2], mode="decrypt")      # (client 1 dropped: extras beside the prepared masks)
        wd = ch.decrypt(want)
        src = torch.from_numpy(np.ascontiguousarray(want).view(signed)).cuda()
        out = torch.empty_like(src)
        assert ct_.decrypt(src, out=out) is out
        got_d = out.cpu().numpy().view(unsigned)
        assert np.array_equal(got_d.astype(np.uint64).reshape(n, -1), wd.astype(np.uint64).reshape(n, -1)), (b, tdt)
        assert ct_.next_iter_decrypt_prepared == ch.next_iter_decrypt_prepared == {}


# ---------------------------------------------------------------- 6. full size
@pytest.mark.parametrize("b,batch", [(20, False), (120, True)])
def test_full_size_precompute_step_against_the_call_by_call_step(b, batch):
    """The 57-layer, 29.2 M-value model as float32 tensors, both directions (the decrypt with extra prefixes), against the call-by-call
    step on the host copies, bit for bit."""
    torch = _torch()
    from flashe_amd import cipher as cm
    cm.N_JOBS = 16
    sizes = [9408] + [s for s in (4096, 16384, 36864, 65536, 147456, 262144, 589824, 1048576, 2359296) for _ in range(6)] + [2048000, 1000]
    g = torch.Generator(device="cuda").manual_seed(0)
    layers = {f"l{i:03d}": torch.randn(s, generator=g, device="cuda", dtype=torch.float32) * 0.05 for i, s in enumerate(sizes)}
    L = 2 if b > 64 else 1
    n_ct = _n_ct(sizes, b, batch, 10)
    res = {}
    for fuse in (True, False):
        cl = _client(b, 10, 3, n_ct, batch=batch, fuse=fuse)
        np.random.seed(8)
        w = cl.quantize_encrypt(_W(dict(layers) if fuse else _host(torch, layers)), device=True)
        ct = w._weights["l000"]
        cl.prepare_decrypt()
        cl.set_idx_list([3])
        if fuse:
            out = {k: torch.empty_like(t, dtype=torch.float64) for k, t in layers.items()}
            cl.decrypt_unquantize(_W({"l000": ct}), out=out)
            back = {k: t.cpu().numpy() for k, t in out.items()}
        else:
            back = cl.decrypt_unquantize(_W({"l000": ct}))._weights
        res[fuse] = (_limbs(ct, L), back)
        del w, ct
    assert np.array_equal(res[True][0], res[False][0])
    for k in layers:
        assert np.asarray(res[True][1][k], dtype=np.float64).tobytes() == np.asarray(res[False][1][k], dtype=np.float64).tobytes(), k
