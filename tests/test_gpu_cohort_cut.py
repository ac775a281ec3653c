"""GPU: a SHORT cohort as one cut chained launch from the floats (FlasheCohort(cut=True): flashe_quantize_encrypt_cohort_cut_dev and its
_u32 form -- prf_chain_cohort_cut_kernel / prf_small_cohort_kernel over several summed chains, then cohort_cut_combine_kernel) against
the reference's recorded client steps and against the same clients run one after the other as FlasheClient steps in one process: every
ciphertext, their sum, NumPy's generator, shape_dict, alpha_list, the floats of decrypt_unquantize and the mean / std history, compared
as bytes.  Outputs and scratch-sized blocks are poisoned first, and `up.path` is asserted everywhere so that a silent mis-route shows.
The pieces each shape is cut into are what csrc/cohort_cut.h gives on the chip the test runs on; they are asserted where the case is about
them."""
import functools
import hashlib
import operator
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden, unhex

pytestmark = pytest.mark.gpu

KEY = bytes(range(32))
try:
    # (asked at collection: once a test has created an engine, the framework of the same process no longer finds its device)
    import torch as _torch_mod
    _TORCH_GPU = _torch_mod.cuda.is_available()
except ImportError:
    _TORCH_GPU = False

COMPACT_WIDTHS = [(16, 12), (20, 16), (23, 16), (24, 16), (32, 24)]            # int_bits, element_bits


class _W:
    def __init__(self, layers):
        self.walking_order = sorted(layers)
        self._weights = dict(layers)


def _arr(hexstr, dtype, shape):
    return np.frombuffer(bytes.fromhex(hexstr), dtype=dtype).copy().reshape(shape)


def _args(b, eb=16):
    return {"quantize": {"int_bits": b, "batch": False, "element_bits": eb, "padding": True, "secure": True}, "precompute": {"enable": False}}


def _poison(eng, sizes):
    """Blocks of the sizes the next call allocates, filled with a pattern and handed back to the engine's pool."""
    bufs = [eng.alloc(max(s, 16)) for s in sizes]
    for b, s in zip(bufs, sizes):
        eng.memset_dev(b, 0xA5, max(s, 16))
    eng.sync()
    for b in bufs:
        b.free()


def _values(dv):
    return np.asarray(dv.to_host(), dtype=np.uint64).reshape(-1)


def _same_state(a, b):
    return a[0] == b[0] and a[2] == b[2] and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ the reference's recorded steps
_DENSE = load_golden("clientstep.json")["dense"]
_RECORDED = [i for i, c in enumerate(_DENSE) if c["scheme"] == "double" and not c.get("batch") and c["b"] in (128, 20, 23)]


@pytest.mark.parametrize("case_i", _RECORDED)
def test_cut_cohort_is_the_reference_jobs_client_steps(case_i):
    """The dense double-mask, un-batched cases of tests/golden/clientstep.json at b = 128 (wide) and b = 20 / 23 (compact=True), recorded by
    calling the reference with per-client seeds, through a cut=True cohort: every flat ciphertext, the element-wise aggregate, alpha,
    shape_dict and the unquantised floats equal the fixture."""
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheCohort
    case = _DENSE[case_i]
    assert len(_RECORDED) == 3
    b, C, compact = case["b"], case["num_clients"], case["b"] <= 32
    cm.N_JOBS = case["n_jobs"]
    co = FlasheCohort(_args(b, case["element_bits"]), first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, compact=compact, cut=True)
    co.set_iter_index(case["iter"])
    ws = [_W({nm: _arr(rec["layers"][nm], np.dtype(dt), sh) for nm, sh, dt in case["layers"]}) for rec in case["clients"]]
    n = sum(int(np.prod(sh)) for _nm, sh, _dt in case["layers"])
    _poison(co.cipher.engine, [(4 if compact else 16) * n] * (C + 3))
    up = co.quantize_encrypt(ws, seeds=[rec["seed"] for rec in case["clients"]])
    assert up.path == "cut-chain" and len(up.ciphertexts) == C
    for c, rec in enumerate(case["clients"]):
        assert [int(v) for v in _ints(up.ciphertexts[c], compact)] == unhex(rec["flat_ct"]), (b, c)
        assert [float(a).hex() for a in co.quantizer.alpha_list] == rec["alpha"]
        assert {k: list(sh) for k, sh in co.shape_dict.items()} == rec["shape_dict"]
    assert [int(v) for v in _ints(up.partial_sum, compact)] == unhex(case["agg_elem"])
    assert (co.lead._cohort_mask is None) == compact
    back = co.decrypt_unquantize()
    assert back.walking_order == sorted(nm for nm, _sh, _dt in case["layers"])
    for nm, sh, _dt in case["layers"]:
        a = back._weights[nm]
        assert a.shape == tuple(sh)
        assert np.asarray(a, dtype=np.float64).tobytes() == bytes.fromhex(case["out_elem"]["unquantized"][nm]), (b, nm)


def _ints(dv, compact):
    from oracle.flashe_oracle import limbs_to_ints
    return _values(dv) if compact else limbs_to_ints(dv.to_host())


# ------------------------------------------------------------------------------------------------ against sequential FlasheClient steps
def _cu_count():
    from flashe_amd import Engine
    return Engine(KEY, 128).cu_count


def _sizes(n):
    """[1, 0, 300, rest]: a layer boundary inside the first pair of lanes' elements, an empty layer, a boundary mid-tile."""
    mid = min(300, n - 1)
    return [1, 0, mid, n - 1 - mid]


def _models(C, sizes, seed, dtypes=("float32", "float64")):
    g = np.random.Generator(np.random.PCG64(seed))
    base = [g.standard_normal(s) * 0.05 for s in sizes]
    return [{f"l{i}": (x + 0.01 * c * np.cos(np.arange(s) + c)).astype(dtypes[i % len(dtypes)]).reshape((s,) if i % 2 else (1, s))
             for i, (x, s) in enumerate(zip(base, sizes))} for c in range(C)]


def _expand(kw, c):
    """The c-th sequential client's kwargs of a cohort call's kwargs (seeds are set by the caller)."""
    out = {}
    if kw.get("rng") is not None:
        out["rng"] = kw["rng"][c] if isinstance(kw["rng"], list) else kw["rng"]
    if kw.get("degrees") is not None:
        out["degree"] = kw["degrees"][c]
    return out


def _rng_states(kw):
    """Where the call left the caller's generators: the next draws of each (asked once, after the round)."""
    r = kw.get("rng")
    return [] if r is None else [g.random(5).tobytes() for g in (r if isinstance(r, list) else [r])]


def _round_trip(b, C, n, compact=False, eb=None, normalize=False, rounds=1, first_idx=0, num_clients=None, want_path="cut-chain", want_parts=None,
                prefer=None, present=None, make_kw=dict, models_of=None, sizes=None, digest=None):
    """`rounds` rounds of a cut=True cohort of C clients against ONE FlasheClient whose cipher takes each client's index in turn (one
    quantiser state, as the cohort has).  make_kw() builds the extra kwargs of the cohort call, called once per side so that both sides
    start from equal generators.  digest: a hashlib object every compared byte also goes into."""
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheClient, FlasheCohort
    cm.N_JOBS = 16
    pos = list(range(C)) if present is None else present
    num_clients = (max(pos) + 1 if num_clients is None else num_clients)
    if eb is None:                                            # (the padded field fits int_bits: element_bits + ceil(log2 num_clients) <= b)
        eb = min(16, b - (num_clients - 1).bit_length())
    sizes = _sizes(n) if sizes is None else sizes
    cl = FlasheClient(_args(b, eb))
    cl.create_cipher(first_idx, num_clients, KEY)
    co = FlasheCohort(_args(b, eb), first_idx=first_idx, n_local=max(pos) + 1 if present is not None else C, num_clients=num_clients, prp_seed=KEY,
                      compact=compact, cut=True)
    co.prefer = prefer
    eng = co.cipher.engine
    elem = 4 if compact else 16
    for it in range(rounds):
        models = (models_of or _models)(C, sizes, 100 + it)
        cl.set_iter_index(it)
        co.set_iter_index(it)
        np.random.seed(7 + it)
        np.random.random(3)                                   # an odd position in the stream
        state = np.random.get_state()
        kw_seq = make_kw()
        want = []
        for c in range(C):
            cl.cipher.idx = first_idx + pos[c]
            if kw_seq.get("seeds") is not None:
                np.random.seed(kw_seq["seeds"][c])
            w = cl.quantize_encrypt(_W(dict(models[c])), device=True, normalize=normalize, **_expand(kw_seq, c))
            want.append(w._weights[w.walking_order[0]])
        cl.cipher.idx = first_idx
        want_state = np.random.get_state()
        want_sum = cl.cipher.aggregate(want)
        plan = co.plan([_W(dict(m)) for m in models], present)
        if want_parts is not None:
            assert plan.parts == want_parts
        _poison(eng, [elem * n] * (C + 2) + [plan.parts * n * elem * (1 if compact else 2)])
        np.random.set_state(state)
        kw = make_kw()
        up = co.quantize_encrypt([_W(dict(m)) for m in models], normalize=normalize, **({} if present is None else {"present": present}), **kw)
        assert up.path == want_path, (up.path, plan.reason)
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
            assert co.lead._cohort_mask is None
        else:
            assert up.partial_sum.to_host().tobytes() == want_sum.to_host().tobytes(), it
        if digest is not None:
            digest.update(_values(up.partial_sum).tobytes())
        assert co.shape_dict == cl.shape_dict
        assert [float(a).hex() for a in co.quantizer.alpha_list] == [float(a).hex() for a in cl.quantizer.alpha_list]
        if num_clients != co.n_local:
            assert co.lead._cohort_mask is None                # clients outside the cohort: no mask is kept
            with pytest.raises(ValueError):
                co.decrypt_unquantize()
            return co
        assert (co.lead._cohort_mask is not None) == (up.path in ("cut-chain", "cohort-chain") and not compact)
        deg = {}
        if kw.get("degrees") is not None:
            deg = {"degree": kw["degrees"][0], "total_degree": functools.reduce(operator.add, kw["degrees"])}
        cl.set_idx_list([first_idx + p for p in pos])
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


def _parts(C, n, b=128, compact=False):
    from flashe_amd.block import cohort_cut_items, cohort_cut_parts
    return cohort_cut_parts(C, cohort_cut_items(n, b, 16, compact), _cu_count())


@pytest.mark.parametrize("C", [1, 2, 3, 17, 40])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 700])
def test_wide_cut_cohort_is_the_sequential_clients(C, n):
    """b = 128: one element, one element short of a tile, a whole tile, one element into the second, three tiles; layers [1, 0, 300, rest]
    in float32 / float64.  Fewer than eight clients are one piece (never fewer than four outputs per piece); 17 clients are four pieces
    of 4, 4, 4 and 5; 40 clients ten pieces of four.  Everything runs in half tiles."""
    _round_trip(128, C, n, want_parts={1: 1, 2: 1, 3: 1, 17: 4, 40: 10}[C])


def test_wide_cut_cohort_at_the_stream_tables_limit():
    """128 clients in 16 pieces: 144 PRF streams, every prefix slot of the launch's table."""
    _round_trip(128, 128, 700, want_parts=16)


def test_wide_cut_cohort_for_three_normalised_rounds():
    _round_trip(128, 3, 700, normalize=True, rounds=3)
    _round_trip(128, 17, 700, normalize=True, rounds=2)


def test_wide_cut_cohort_below_two_limbs_of_mask():
    """int_bits 65: the mask words of the pieces' sums and masks and of the combine pass."""
    _round_trip(65, 5, 700)
    _round_trip(65, 17, 700, want_parts=4)


def test_config_3s_own_shape():
    """LeNet's 61,706 values x 100 clients (BASELINE config 3) at b = 128."""
    _round_trip(128, 100, 61706, want_parts=_parts(100, 61706))


def test_one_element_below_the_admission_length_is_one_piece():
    """Almost two whole tiles per wave: "cut-chain" with one piece -- one launch, no scratch, no combine pass; at the admission length itself
    the uncut chain runs as before."""
    from flashe_amd.block import cohort_admission_length
    n = cohort_admission_length(_cu_count())
    co = _round_trip(128, 3, n - 1, normalize=True, want_parts=1)
    assert co._cut_scratch is None
    _round_trip(128, 3, n, normalize=True, want_path="cohort-chain")


def test_a_cut_cohort_inside_a_larger_federation_writes_a_partial_aggregate():
    _round_trip(128, 4, 700, first_idx=3, num_clients=9)
    _round_trip(128, 20, 700, first_idx=3, num_clients=40, want_parts=5)
    _round_trip(20, 20, 700, compact=True, first_idx=3, num_clients=40)


@pytest.mark.parametrize("b,eb", COMPACT_WIDTHS)
def test_compact_cut_cohort_at_every_width(b, eb):
    _round_trip(b, 5, 700, compact=True, eb=eb, normalize=True)
    _round_trip(b, 17, 700, compact=True, want_parts=4)


@pytest.mark.parametrize("n", [1, 5, 6 * 128 * 3 + 1])
def test_compact_cut_cohort_at_chunk_and_tile_edges(n):
    """int_bits 20 (m = 6): n < N_JOBS -- chunks of zero and one element, every block partial -- and one element past three tiles' worth of
    whole blocks."""
    _round_trip(20, 5, n, compact=True)
    _round_trip(20, 17, n, compact=True, want_parts=4)


@pytest.mark.parametrize("C,n", [(17, 700), (128, 700), (100, 61706)])
def test_compact_cut_cohort_many_clients(C, n):
    _round_trip(20, C, n, compact=True, want_parts=_parts(C, n, 20, True))
    assert _parts(128, 700, 20, True) == 16 and _parts(17, 700, 20, True) == 4


# ------------------------------------------------------------------------------------------------ what rides on the tables and the draws
def test_seeds_on_the_cut_path():
    _round_trip(128, 3, 700, make_kw=lambda: {"seeds": [5, 6, 7]})
    _round_trip(128, 17, 700, make_kw=lambda: {"seeds": list(range(30, 47))})


def test_one_generator_and_a_list_of_philox_generators():
    _round_trip(128, 3, 700, make_kw=lambda: {"rng": np.random.default_rng(11)})
    _round_trip(128, 3, 700, make_kw=lambda: {"rng": [np.random.Generator(np.random.Philox(key=40 + c)) for c in range(3)]})
    _round_trip(20, 17, 700, compact=True, make_kw=lambda: {"rng": np.random.default_rng(12)})


def test_degrees_on_the_cut_path():
    _round_trip(128, 3, 700, normalize=True, make_kw=lambda: {"degrees": [3, 5, 2]})
    _round_trip(128, 17, 700, make_kw=lambda: {"degrees": [1 + c % 4 for c in range(17)]})


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_framework_tensors_on_the_cut_path(dtype):
    torch = pytest.importorskip("torch")
    if not (_TORCH_GPU and torch.cuda.is_available()):
        pytest.skip("no GPU visible to torch")

    def tensors(C, sizes, seed):
        return [{k: torch.from_numpy(np.asarray(v, dtype=np.float32)).to("cuda").to(getattr(torch, dtype)) for k, v in m.items()}
                for m in _models(C, sizes, seed, dtypes=("float32",))]
    # (no empty layer here: the framework hands an empty tensor over with stride 0)
    _round_trip(128, 3, 700, normalize=True, models_of=tensors, sizes=[1, 300, 399])
    _round_trip(20, 17, 700, compact=True, models_of=tensors, sizes=[1, 300, 399])


def test_present_everyone_is_the_plain_call_and_a_gap_runs_staged():
    a, b = hashlib.sha256(), hashlib.sha256()
    _round_trip(128, 3, 700, digest=a)
    _round_trip(128, 3, 700, present=[0, 1, 2], digest=b)
    assert a.digest() == b.digest()
    _round_trip(128, 2, 700, present=[0, 2], want_path="staged-chain")


def test_prefer_staged_gives_the_same_bytes():
    for kw in ({"C": 17, "b": 128}, {"C": 17, "b": 20, "compact": True}):
        a, b = hashlib.sha256(), hashlib.sha256()
        _round_trip(kw["b"], kw["C"], 700, compact=kw.get("compact", False), digest=a)
        _round_trip(kw["b"], kw["C"], 700, compact=kw.get("compact", False), prefer="staged-chain", want_path="staged-chain", digest=b)
        assert a.digest() == b.digest()


def _child():
    d = hashlib.sha256()
    _round_trip(128, 17, 700, want_path=os.environ["WANT_PATH"], digest=d)
    print("DIGEST", d.hexdigest())


def test_flashe_chain_0_runs_staged_with_the_same_bytes():
    """FLASHE_CHAIN=0 is read when the engine is created: a child process runs the same cut=True cohort on the staged form."""
    d = hashlib.sha256()
    _round_trip(128, 17, 700, digest=d)
    code = "import sys; sys.path.insert(0, %r); import test_gpu_cohort_cut as t; t._child()" % os.path.join(ROOT, "tests")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, FLASHE_CHAIN="0", WANT_PATH="staged-chain"))
    assert r.returncode == 0 and "DIGEST " + d.hexdigest() in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ------------------------------------------------------------------------------------------------ the raw entry points
def _raw(eng, C, n, compact, bits=16):
    """One shared float32 row, every client reading the same source: the arguments of the cut entry points and their outputs."""
    from flashe_amd import _lib
    elem = 4 if compact else 16
    x, u = eng.upload(np.linspace(-0.4, 0.4, n).astype(np.float32)), eng.upload(np.random.Generator(np.random.PCG64(1)).random(C * n))
    rows, srcs, dts = [(0, None, 0.5, 0.0, _lib.TENSOR_F32, 0)], [[x.ptr]] * C, [[_lib.TENSOR_F32]] * C
    cts, dsum, dmask = [eng.alloc(elem * n) for _ in range(C)], eng.alloc(elem * n), eng.alloc(elem * n)
    for d in cts + [dsum, dmask]:
        eng.memset_dev(d, 0xA5, elem * n)
    return (3, 0, n, 16, rows, srcs, dts, bits, u, cts, dsum), dmask, (x, u)


def _untouched(eng, bufs, n, elem):
    eng.sync()
    return all((d.download(np.uint8, elem * n) == 0xA5).all() for d in bufs)


def test_the_raw_entry_points_refuse_a_bad_scratch():
    from flashe_amd import engine as E
    n, C = 700, 17
    for compact, b in ((False, 128), (True, 20)):
        eng = E.Engine(KEY, b, device=0)
        elem = 4 if compact else 16
        parts = eng.cohort_cut_parts(C, n, 16, compact=compact)
        assert parts == 4
        a, dmask, _keep = _raw(eng, C, n, compact)
        call = eng.quantize_encrypt_cohort_cut_u32_dev if compact else functools.partial(eng.quantize_encrypt_cohort_cut_dev, dmask=dmask)
        scratch = eng.alloc(2 * parts * n * elem + 64)
        for bad in (None, E.DeviceBufferView(scratch, 8, parts * n * elem), a[9][0], a[10]) + (() if compact else (dmask,)):
            with pytest.raises(E.FlasheError) as ei:
                call(*a, scratch=bad)
            assert ei.value.code == -22
        assert _untouched(eng, a[9] + [a[10], dmask], n, elem)
        assert call(*a, scratch=scratch) is True
        eng.sync()
        assert not (a[10].download(np.uint8, elem * n) == 0xA5).all()
        # one piece: no scratch is needed
        a1, dmask1, _keep1 = _raw(eng, 3, n, compact)
        assert eng.cohort_cut_parts(3, n, 16, compact=compact) == 1
        call1 = eng.quantize_encrypt_cohort_cut_u32_dev if compact else functools.partial(eng.quantize_encrypt_cohort_cut_dev, dmask=dmask1)
        assert call1(*a1, scratch=None) is True


def test_the_raw_entry_points_decline_what_the_launch_does_not_take():
    from flashe_amd import engine as E
    n = 700
    eng = E.Engine(KEY, 128, device=0)
    a, dmask, _keep = _raw(eng, 129, n, False)
    scratch = eng.alloc(2 * 16 * n * 16)
    assert eng.cohort_cut_parts(129, n, 16) == 0 and eng.cohort_cut_parts(128, n, 16) == 16
    assert eng.quantize_encrypt_cohort_cut_dev(*a, dmask=dmask, scratch=scratch) is False
    assert _untouched(eng, a[9] + [a[10], dmask], n, 16)
    for b in (64, 33):
        e64 = E.Engine(KEY, b, device=0)
        a, dmask, _keep = _raw(e64, 3, n, False)
        assert e64.cohort_cut_parts(3, n, 16) == 0 and e64.cohort_cut_parts(3, n, 16, compact=True) == 0
        assert e64.quantize_encrypt_cohort_cut_dev(*a, scratch=e64.alloc(4096)) is False
        assert _untouched(e64, a[9] + [a[10]], n, 16)
    e21 = E.Engine(KEY, 21, device=0)                       # the compact layout without a compiled-in chain
    a, _dmask, _keep = _raw(e21, 3, n, True)
    assert e21.quantize_encrypt_cohort_cut_u32_dev(*a, scratch=e21.alloc(4096)) is False
    assert _untouched(e21, a[9] + [a[10]], n, 4)
