"""GPU, class level: rng= over np.random.PCG64 -- what np.random.default_rng returns -- and np.random.PCG64DXSM on FlasheClient, FlasheCohort
and FlasheSparseCohort, on the steps and the reference form of tests/test_gpu_rng_argument.py: the SAME call with FLASHE_DEVICE_RNG=0 and
np.random.random replaced, for the duration of the call, by the .random of identically constructed generators -- the host-draw path.
Compared as bytes: every ciphertext, the partial sum or aggregate, alpha_list, shape_dict and the generators' states afterwards
(has_uint32 / uinteger included: the generators start with a cached 32-bit word); NumPy's global stream must be left alone.  The models
hold 70,001 values, just over DEVICE_RNG_MIN, so the generators draw on the device, asserted by counting Engine.pcg64_random_dev calls:
ONE per call whatever the number of clients and whichever of the two variants they hold; a list that mixes Philox, PCG64, PCG64DXSM and
SFC64 is one Philox launch, one PCG launch and one host stretch; one cohort case runs at the chained launch's admission length so that the
chain itself reads the one-launch draws."""
import numpy as np
import pytest

from test_gpu_rng_argument import COHORTS, KEY, N, SIZES, _client_step, _cohort_step, _global, _patched, _sparse_step, _state

pytestmark = pytest.mark.gpu

BITGENS = {"PCG64": np.random.PCG64, "PCG64DXSM": np.random.PCG64DXSM, "Philox": np.random.Philox, "SFC64": np.random.SFC64}


def _gen(seed, kind="default_rng"):
    """default_rng(seed) itself, or a Generator over the named bit generator; a 32-bit draw taken, so that has_uint32 = 1 and the cached word
    has to survive the device call."""
    g = np.random.default_rng(seed) if kind == "default_rng" else np.random.Generator(BITGENS[kind](seed))
    g.integers(0, 2 ** 32, dtype=np.uint32)
    return g


def _pair(seeds, kinds):
    return [_gen(s, k) for s, k in zip(seeds, kinds)], [_gen(s, k) for s, k in zip(seeds, kinds)]


@pytest.fixture
def pcg_calls(monkeypatch):
    """The segment counts of every Engine.pcg64_random_dev call, on whichever engine."""
    from flashe_amd import Engine
    calls, fn = [], Engine.pcg64_random_dev

    def call(self, gens, counts, **kw):
        calls.append(list(counts))
        return fn(self, gens, counts, **kw)
    monkeypatch.setattr(Engine, "pcg64_random_dev", call)
    return calls


def test_default_rng_is_the_generator_the_device_call_takes():
    assert isinstance(np.random.default_rng(1).bit_generator, np.random.PCG64)


# ---------------------------------------------------------------------------------------------------------------------- FlasheClient
@pytest.mark.parametrize("b, batch, zzz", [(128, False, False), (120, True, False), (20, False, False), (128, False, True), (20, False, True)],
                         ids=["128", "120-batched", "20", "128-sparse-job", "20-sparse-job"])
@pytest.mark.parametrize("kind", ["default_rng", "PCG64DXSM"])
def test_the_client_step_draws_from_the_generator_on_the_device(monkeypatch, pcg_calls, b, batch, zzz, kind):
    np.random.seed(1)
    before = _global()
    (ref_g,), (g,) = _pair([77], [kind])
    want, _c = _patched(monkeypatch, [ref_g], N, lambda: _client_step(b, batch, zzz, None))
    assert pcg_calls == []
    got, philox = _client_step(b, batch, zzz, g)
    assert got == want
    assert pcg_calls == [[N]] and philox == []                      # ONE launch for the model's draws; the 'zzz' draw is a host draw
    assert _state(g) == _state(ref_g) and g.bit_generator.state["has_uint32"] == 1 and _global() == before
    assert g.integers(0, 2 ** 32, 2, dtype=np.uint32).tobytes() == ref_g.integers(0, 2 ** 32, 2, dtype=np.uint32).tobytes()
    assert g.random(5).tobytes() == ref_g.random(5).tobytes()


# ---------------------------------------------------------------------------------------------------------------------- FlasheCohort
@pytest.mark.parametrize("setting", list(COHORTS))
@pytest.mark.parametrize("form", ["one", "list"])
def test_the_cohort_draws_from_the_generators_in_one_launch(monkeypatch, pcg_calls, setting, form):
    b, batch, compact, present = COHORTS[setting]
    C = 3 if present is None else len(present)
    seeds = [31] if form == "one" else [31, 32, 33][:C]
    kinds = ["default_rng", "PCG64DXSM", "PCG64"][:len(seeds)]      # the two variants share the launch
    np.random.seed(2)
    before = _global()
    refs, gens = _pair(seeds, kinds)
    want, _c = _patched(monkeypatch, refs, N, lambda: _cohort_step(b, batch, compact, C, SIZES, present, None))
    assert pcg_calls == []
    got, philox = _cohort_step(b, batch, compact, C, SIZES, present, gens[0] if form == "one" else gens)
    assert got == want
    assert pcg_calls == ([[C * N]] if form == "one" else [[N] * C]) and philox == []      # ONE call: one stretch, or a segment per client
    assert [_state(g) for g in gens] == [_state(r) for r in refs] and _global() == before
    for g, r in zip(gens, refs):
        assert g.integers(0, 2 ** 32, 2, dtype=np.uint32).tobytes() == r.integers(0, 2 ** 32, 2, dtype=np.uint32).tobytes()


def test_a_mixed_list_is_one_launch_per_kind_and_one_host_stretch(monkeypatch, pcg_calls):
    kinds, seeds = ["Philox", "default_rng", "PCG64DXSM", "SFC64"], [51, 52, 53, 54]
    np.random.seed(4)
    before = _global()
    refs, gens = _pair(seeds, kinds)
    want, _c = _patched(monkeypatch, refs, N, lambda: _cohort_step(128, False, False, 4, SIZES, None, None))
    assert pcg_calls == []
    got, philox = _cohort_step(128, False, False, 4, SIZES, None, gens)
    assert got == want
    assert philox == [[N]] and pcg_calls == [[N, N]]                # the SFC64 client's stretch is the host's: its state below says it drew
    assert [_state(g) for g in gens] == [_state(r) for r in refs] and _global() == before


def test_the_chained_launch_reads_the_one_launch_draws(monkeypatch, pcg_calls):
    from flashe_amd import Engine
    from flashe_amd.block import cohort_admission_length
    n = cohort_admission_length(Engine(KEY, 128).cu_count)
    sizes = [n - 1000, 0, 1000]
    refs, gens = _pair([41, 42], ["default_rng", "PCG64DXSM"])
    np.random.seed(3)
    before = _global()
    want, _c = _patched(monkeypatch, refs, n, lambda: _cohort_step(128, False, False, 2, sizes, None, None, "cohort-chain"))
    got, philox = _cohort_step(128, False, False, 2, sizes, None, gens, "cohort-chain")
    assert got == want and pcg_calls == [[n, n]] and philox == []
    assert [_state(g) for g in gens] == [_state(r) for r in refs] and _global() == before


# ---------------------------------------------------------------------------------------------------------------------- FlasheSparseCohort
@pytest.mark.parametrize("form", ["one", "list"])
def test_the_sparse_cohort_draws_from_the_generators(monkeypatch, pcg_calls, form):
    seeds = [61] if form == "one" else [61, 62, 63]
    refs, gens = _pair(seeds, ["default_rng", "PCG64DXSM", "PCG64"][:len(seeds)])
    np.random.seed(5)
    before = _global()
    want, _c = _patched(monkeypatch, refs, 70001, lambda: _sparse_step(None))
    assert pcg_calls == []
    got, philox = _sparse_step(gens[0] if form == "one" else gens)
    assert got == want
    assert pcg_calls == ([[3 * 70001]] if form == "one" else [[70001] * 3]) and philox == []     # the odd K + 1 stride: 8-byte aligned only
    assert [_state(g) for g in gens] == [_state(r) for r in refs] and _global() == before


# ---------------------------------------------------------------------------------------------------------------------- the quantiser alone
def test_the_static_quantiser_and_the_environment_switch(monkeypatch, pcg_calls):
    from flashe_amd.quantize import _static_quantize_padding_asymmetric
    x = (np.random.Generator(np.random.PCG64(3)).standard_normal(N) * 0.05).astype(np.float32)
    (ref,), (g,) = _pair([9], ["default_rng"])
    want = _static_quantize_padding_asymmetric(x, 0.2, 16, uniforms=ref.random(N), as_object=False)
    got = _static_quantize_padding_asymmetric(x, 0.2, 16, rng=g, as_object=False)
    assert got.tobytes() == want.tobytes() and pcg_calls == [[N]] and _state(g) == _state(ref)
    monkeypatch.setenv("FLASHE_DEVICE_RNG", "0")                    # the same generator draws on the host
    want = _static_quantize_padding_asymmetric(x, 0.2, 16, uniforms=ref.random(N), as_object=False)
    got = _static_quantize_padding_asymmetric(x, 0.2, 16, rng=g, as_object=False)
    assert got.tobytes() == want.tobytes() and pcg_calls == [[N]] and _state(g) == _state(ref)
    monkeypatch.delenv("FLASHE_DEVICE_RNG")
    short = x[:65535]                                               # one below DEVICE_RNG_MIN: a host draw
    want = _static_quantize_padding_asymmetric(short, 0.2, 16, uniforms=ref.random(65535), as_object=False)
    got = _static_quantize_padding_asymmetric(short, 0.2, 16, rng=g, as_object=False)
    assert got.tobytes() == want.tobytes() and pcg_calls == [[N]] and _state(g) == _state(ref)
