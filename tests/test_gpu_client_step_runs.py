"""GPU: FlasheClient's fused step cut into runs of whole layers (flashe_amd/block.py, _encrypt_tail: at most _RNG_RUN_MAX draws per run, 2^26
in production) against the same call with the run length left alone -- one launch.  Five layers of 4, 3, 0, 6 and 2 values with the run
length at 5 are the smallest model at which the loop can go wrong: runs (0, 4), (4, 3), (7, 6), (13, 2), a lone layer over the cap, an
empty layer, and at int_bits 20 every run but the first starts inside an AES block of six elements (two chunks: blocks 0-5, 6-7, 8-13,
14).  The ranges of the entry points themselves are test_gpu_codec_edges.py's: a difference here is a finding about the Python loop."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEY = bytes(range(32))
SIZES = [4, 3, 0, 6, 2]
N = sum(SIZES)

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


def _layers(source):
    """The five layers as host float32 arrays, or as torch device tensors of dtype `source` holding the same values."""
    rng = np.random.Generator(np.random.PCG64(11))
    host = {f"l{i}": rng.standard_normal(s).astype(np.float16).astype(np.float32) for i, s in enumerate(SIZES)}      # (exact in every dtype)
    if source == "host":
        return host
    torch = pytest.importorskip("torch")
    if not (_TORCH_GPU and torch.cuda.is_available()):
        pytest.skip("no GPU visible to torch")
    out = {k: torch.empty(v.shape, dtype=getattr(torch, source), device="cuda").copy_(torch.from_numpy(v)) for k, v in host.items()}
    torch.cuda.synchronize()
    return out


def _step(monkeypatch, run_max, b, scheme, source, prepared, zzz):
    from flashe_amd import block, cipher as cm
    from flashe_amd.block import FlasheClient
    monkeypatch.setattr(cm, "N_JOBS", 2)
    args = {"quantize": {"int_bits": b, "batch": False, "element_bits": 16, "padding": True, "secure": True},
            "precompute": {"enable": prepared, "num_params": N}}
    cl = FlasheClient(args)
    cl.create_cipher(1, 3, KEY)
    cl.cipher.masking_scheme = scheme
    if prepared:
        cl.set_iter_index(4)
        cl.prepare_encrypt()
    cl.set_iter_index(5)
    layers = _layers(source)
    if zzz:
        layers["zzz"] = np.array([0.3], dtype=np.float32)
    with monkeypatch.context() as m:
        if run_max is not None:
            m.setattr(block, "_RNG_RUN_MAX", run_max)
        np.random.seed(29)
        res = cl.quantize_encrypt(_W(layers), device=True)
    st = np.random.get_state()
    assert list(res._weights) == ["l0"]
    held = cl.cipher.engine.prepared_query(cl.cipher.engine.PREPARED_ENCRYPT)[0]
    return (res._weights["l0"].to_host().tobytes(), cl.shape_dict, list(cl.quantizer.alpha_list), (st[0], st[1].tobytes(), st[2]),
            sorted(cl.cipher.next_iter_encrypt_prepared), held)


def _compare(monkeypatch, b, scheme, source, prepared, zzz):
    cut = _step(monkeypatch, 5, b, scheme, source, prepared, zzz)
    whole = _step(monkeypatch, None, b, scheme, source, prepared, zzz)
    n_out = N + (1 if zzz else 0)
    assert len(whole[0]) == n_out * 8 * (2 if b > 64 else 1)
    assert cut[0] == whole[0], "the ciphertexts of the cut and the uncut step differ"
    assert cut[1] == whole[1] == {f"l{i}": (s,) for i, s in enumerate(SIZES)}
    assert cut[2] == whole[2] and len(cut[2]) == 5
    np.random.seed(29)
    np.random.random(n_out)
    st = np.random.get_state()
    assert cut[3] == whole[3] == (st[0], st[1].tobytes(), st[2])               # one draw per value, 'zzz' included
    assert cut[4:] == whole[4:]
    return cut


@pytest.mark.parametrize("source", ["host", "float32", "float64", "float16"])
@pytest.mark.parametrize("prepared", [False, True], ids=["online", "prepared"])
@pytest.mark.parametrize("scheme", ["double", "single"])
@pytest.mark.parametrize("b", [128, 64, 20])
def test_the_cut_step_is_the_uncut_step(monkeypatch, b, scheme, prepared, source):
    cut = _compare(monkeypatch, b, scheme, source, prepared, False)
    if prepared and scheme == "double":
        assert cut[4:] == ([], False), "the run that ends the vector consumes the cache"       # (mode "ctx")
    elif prepared:
        assert cut[4:] == (["minus"], True)         # (a single-mask cipher does not read the cache: it drops 'add' as the reference does)


@pytest.mark.parametrize("source", ["host", "float32"])
@pytest.mark.parametrize("scheme", ["double", "single"])
@pytest.mark.parametrize("b", [128, 64, 20])
def test_the_sparse_jobs_cut_step_is_the_uncut_step(monkeypatch, b, scheme, source):
    _compare(monkeypatch, b, scheme, source, False, True)
