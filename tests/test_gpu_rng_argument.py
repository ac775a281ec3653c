"""GPU, class level: rng= on FlasheClient, FlasheCohort and FlasheSparseCohort.  The reference form of every call is the SAME call with
FLASHE_DEVICE_RNG=0 and np.random.random replaced, for the duration of the call, by the .random of identically constructed generators --
the host-draw path, which consumes np.random.random only.  Compared as bytes: every ciphertext, the partial sum or aggregate, alpha_list,
shape_dict and the generators' states afterwards; NumPy's global stream must be left alone.  The models hold 70,001 values, just over
DEVICE_RNG_MIN, so Philox generators draw on the device (asserted by counting the engine's philox_random_dev calls: ONE per cohort call
whatever the number of clients); one cohort case runs at the chained launch's admission length so that the chain itself reads the
one-launch draws."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEY = bytes(range(32))
SIZES = [10007, 59993, 1]                          # 70,001 values in three layers
N = sum(SIZES)


class _W:
    def __init__(self, layers):
        self.walking_order = sorted(layers)
        self._weights = dict(layers)


def _args(b, batch=False, mask=None):
    a = {"quantize": {"int_bits": b, "batch": batch, "element_bits": 16, "padding": True, "secure": True}, "precompute": {"enable": False, "num_params": 11}}
    if mask:
        a["mask"] = mask
    return a


def _models(C, sizes, seed=5):
    g = np.random.Generator(np.random.PCG64(seed))
    return [{f"l{i}": (g.standard_normal(s) * 0.05 + 0.01 * c).astype(np.float64 if i == 1 else np.float32) for i, s in enumerate(sizes)}
            for c in range(C)]


def _gens(bitgen, seeds):
    return [np.random.Generator(bitgen(s)) for s in seeds]


def _state(g):
    st = g.bit_generator.state
    flat = list(st.items()) + list(st["state"].items())
    return sorted((k, v.tobytes() if isinstance(v, np.ndarray) else repr(v)) for k, v in flat if not isinstance(v, dict))


def _global():
    st = np.random.get_state()
    return st[1].tobytes(), st[2]


class _Count:
    """Counts an engine's philox_random_dev calls and their segments."""

    def __init__(self, eng):
        self.calls, fn = [], eng.philox_random_dev

        def call(gens, counts, **kw):
            self.calls.append(list(counts))
            return fn(gens, counts, **kw)
        eng.philox_random_dev = call


def _patched(monkeypatch, refs, stretch, call):
    """call() with FLASHE_DEVICE_RNG=0 and np.random.random drawing from refs: one generator -- every request goes to it; a list -- a
    request for len(refs) stretches is the clients' stretches one after the other, client c's from refs[c]."""
    def random(size=None):
        count = int(np.prod(size)) if size is not None else 1
        if len(refs) == 1:
            return refs[0].random(size)
        assert count == len(refs) * stretch, (count, stretch)
        return np.concatenate([r.random(stretch) for r in refs])
    with monkeypatch.context() as m:
        m.setenv("FLASHE_DEVICE_RNG", "0")
        m.setattr(np.random, "random", random)
        return call()


# ---------------------------------------------------------------------------------------------------------------------- FlasheClient
def _client_step(b, batch, zzz, rng):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheClient
    cm.N_JOBS = 16
    cl = FlasheClient(_args(b, batch))
    cl.create_cipher(1, 3, KEY)
    cl.set_iter_index(2)
    layers = dict(_models(1, SIZES)[0])
    if zzz:
        layers["zzz"] = np.array([0.3], dtype=np.float32)
    count = _Count(cl.cipher.engine)
    res = cl.quantize_encrypt(_W(layers), device=True, normalize=True, rng=rng)
    ct = res._weights[res.walking_order[0]]
    return (ct.to_host().tobytes(), [float(a).hex() for a in cl.quantizer.alpha_list], dict(cl.shape_dict)), count.calls


@pytest.mark.parametrize("b, batch, zzz", [(128, False, False), (120, True, False), (20, False, False), (128, False, True), (20, False, True)],
                         ids=["128", "120-batched", "20", "128-sparse-job", "20-sparse-job"])
@pytest.mark.parametrize("bitgen", [np.random.Philox, np.random.PCG64], ids=["philox", "pcg64"])
def test_the_client_step_draws_from_the_generator(monkeypatch, b, batch, zzz, bitgen):
    np.random.seed(1)
    before = _global()
    (ref_g,), (g,) = _gens(bitgen, [77]), _gens(bitgen, [77])
    g.random(2), ref_g.random(2)                                    # an odd position: buffer_pos 2
    want, _c = _patched(monkeypatch, [ref_g], N, lambda: _client_step(b, batch, zzz, None))
    got, calls = _client_step(b, batch, zzz, g)
    assert got == want
    assert calls == ([[N]] if bitgen is np.random.Philox else [])     # the device generated the model's draws; the 'zzz' draw is a host draw
    assert _state(g) == _state(ref_g) and _global() == before
    twin = _gens(bitgen, [77])[0]
    twin.random(2 + N + (1 if zzz else 0))
    assert g.random(5).tobytes() == twin.random(5).tobytes()


# ---------------------------------------------------------------------------------------------------------------------- FlasheCohort
def _cohort_step(b, batch, compact, C, sizes, present, rng, want_path=None):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheCohort
    cm.N_JOBS = 16
    n_local = C if present is None else max(present) + 1
    co = FlasheCohort(_args(b, batch), first_idx=0, n_local=n_local, num_clients=n_local, prp_seed=KEY, compact=compact)
    co.set_iter_index(3)
    count = _Count(co.cipher.engine)
    up = co.quantize_encrypt([_W(dict(m)) for m in _models(C, sizes)], normalize=True, present=present, rng=rng)
    if want_path is not None:
        assert up.path == want_path
    return ([v.to_host().tobytes() for v in up.ciphertexts], up.partial_sum.to_host().tobytes(), [float(a).hex() for a in co.quantizer.alpha_list],
            dict(co.shape_dict), up.path, up.present), count.calls


COHORTS = {"128": (128, False, False, None), "dropout": (128, False, False, [0, 2]), "20-compact": (20, False, True, None),
           "120-batched": (120, True, False, None)}


@pytest.mark.parametrize("setting", list(COHORTS))
@pytest.mark.parametrize("form", ["one", "list"])
def test_the_cohort_draws_from_the_generators_in_one_launch(monkeypatch, setting, form):
    b, batch, compact, present = COHORTS[setting]
    C = 3 if present is None else len(present)
    seeds = [31] if form == "one" else [31, 32, 33][:C]
    np.random.seed(2)
    before = _global()
    refs, gens = _gens(np.random.Philox, seeds), _gens(np.random.Philox, seeds)
    want, _c = _patched(monkeypatch, refs, N, lambda: _cohort_step(b, batch, compact, C, SIZES, present, None))
    got, calls = _cohort_step(b, batch, compact, C, SIZES, present, gens[0] if form == "one" else gens)
    assert got == want
    assert calls == ([[C * N]] if form == "one" else [[N] * C])       # ONE launch: one stretch, or a segment per client
    assert [_state(g) for g in gens] == [_state(r) for r in refs] and _global() == before


def test_the_chained_launch_reads_the_one_launch_draws(monkeypatch):
    from flashe_amd import Engine
    from flashe_amd.block import cohort_admission_length
    n = cohort_admission_length(Engine(KEY, 128).cu_count)
    sizes = [n - 1000, 0, 1000]
    refs, gens = _gens(np.random.Philox, [41, 42]), _gens(np.random.Philox, [41, 42])
    np.random.seed(3)
    before = _global()
    want, _c = _patched(monkeypatch, refs, n, lambda: _cohort_step(128, False, False, 2, sizes, None, None, "cohort-chain"))
    got, calls = _cohort_step(128, False, False, 2, sizes, None, gens, "cohort-chain")
    assert got == want and calls == [[n, n]]
    assert [_state(g) for g in gens] == [_state(r) for r in refs] and _global() == before


def test_a_pcg64_cohort_draws_on_the_host(monkeypatch):
    refs, gens = _gens(np.random.PCG64, [51, 52, 53]), _gens(np.random.PCG64, [51, 52, 53])
    np.random.seed(4)
    before = _global()
    want, _c = _patched(monkeypatch, refs, N, lambda: _cohort_step(128, False, False, 3, SIZES, None, None))
    got, calls = _cohort_step(128, False, False, 3, SIZES, None, gens)
    assert got == want and calls == []
    assert [_state(g) for g in gens] == [_state(r) for r in refs] and _global() == before


# ---------------------------------------------------------------------------------------------------------------------- FlasheSparseCohort
def _sparse_step(rng, K=70000, total=200000, C=3):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheSparseCohort
    cm.N_JOBS = 16
    ks = (10007, 59992, 1)
    assert sum(ks) == K
    g = np.random.Generator(np.random.PCG64(9))
    co = FlasheSparseCohort(_args(20, mask="dynamic"), first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, sparsity=0.35)
    co.set_iter_index(2)
    lists = [np.sort(g.choice(total, K, replace=False)) for _ in range(C)]
    assert co.dynamic_masking("single", [l.tolist() for l in lists], total) == "single"
    compact = [{f"l{i}": (g.standard_normal(k) * 0.05).astype(np.float64 if i == 1 else np.float32) for i, k in enumerate(ks)} for _ in range(C)]
    count = _Count(co.engine)
    up = co.quantize_encrypt(compact=compact, normalize=True, rng=rng)
    assert up.path == "sparse-cohort" and up.front_end == "fused"
    return ([u.to_host().tobytes() for u in up.uploads], up.aggregate.to_host().tobytes(), [float(a).hex() for a in co.quantizer.alpha_list],
            dict(co.shape_dict)), count.calls


@pytest.mark.parametrize("form", ["one", "list"])
def test_the_sparse_cohort_draws_from_the_generators(monkeypatch, form):
    seeds = [61] if form == "one" else [61, 62, 63]
    refs, gens = _gens(np.random.Philox, seeds), _gens(np.random.Philox, seeds)
    np.random.seed(5)
    before = _global()
    want, _c = _patched(monkeypatch, refs, 70001, lambda: _sparse_step(None))
    got, calls = _sparse_step(gens[0] if form == "one" else gens)
    assert got == want
    assert calls == ([[3 * 70001]] if form == "one" else [[70001] * 3])     # the odd K + 1 stride: client 1's stretch is 8-byte aligned only
    assert [_state(g) for g in gens] == [_state(r) for r in refs] and _global() == before
