"""GPU, class level: a precompute job's FlasheCohort(inline_draws="any") whose rng= generators are np.random.default_rng's draws INSIDE its
online launch under FLASHE_INLINE_DRAWS=1 (CohortUpload.draws == "inline": no draw buffer) -- every ciphertext, the sum,
decrypt_unquantize's floats and the generators' final states against a second identical cohort run with FLASHE_INLINE_DRAWS=0 ("buffer":
the draws materialised in HBM first).  inline_draws=True and the default cohort, a batched job and a list of PCG64 and Philox generators
keep the buffer; with the switch unset the layout's entry of _INLINE_PCG64_DEFAULT decides."""
import copy

import numpy as np
import pytest

from test_gpu_cohort import KEY, _host_models
from test_gpu_cohort_prepared_class import IT, SIZES, _args, _n_ct, _vals
from test_gpu_cohort_prepared_philox_class import _round

pytestmark = pytest.mark.gpu

C = 10


def _cohort(b, batch, compact, **kw):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheCohort
    cm.N_JOBS = 16
    co = FlasheCohort(_args(b, batch, _n_ct(SIZES, b, batch, C)), first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, compact=compact, **kw)
    co.set_iter_index(IT - 1)
    co.prepare_encrypt()
    co.set_iter_index(IT)
    return co


def _rngs(kind):
    if kind == "one":
        g = np.random.default_rng(7)
        g.random(3)                                                   # an odd position in the stream
        return g, None
    if kind == "list":
        gens = [np.random.default_rng(7 + c) for c in range(C)]
        for c, g in enumerate(gens):
            g.random(c)
        return gens, None
    g = np.random.default_rng(7)
    g.random(2)
    return g, [0, 1, 3, 4, 5, 6, 8, 9]


@pytest.mark.parametrize("kind", ["one", "list", "present"])
@pytest.mark.parametrize("b,compact", [(128, False), (20, True)])
def test_inline_draws_are_the_buffer_forms_bytes(monkeypatch, b, compact, kind):
    models = _host_models(C, SIZES, 11)
    rng, present = _rngs(kind)
    other = copy.deepcopy(rng)
    monkeypatch.delenv("FLASHE_DEVICE_RNG", raising=False)
    monkeypatch.setenv("FLASHE_INLINE_DRAWS", "1")
    up, floats = _round(_cohort(b, False, compact, inline_draws="any"), models, rng, present)
    assert up.draws == "inline"
    monkeypatch.setenv("FLASHE_INLINE_DRAWS", "0")
    want, want_floats = _round(_cohort(b, False, compact, inline_draws="any"), models, other, present)
    assert want.draws == "buffer"
    assert up.present == want.present and len(up.ciphertexts) == len(want.ciphertexts) == (C if present is None else len(present))
    for c in range(len(want.ciphertexts)):
        assert up.ciphertexts[c].compact == compact
        assert _vals(up.ciphertexts[c]).tobytes() == _vals(want.ciphertexts[c]).tobytes(), (kind, c)
    assert _vals(up.partial_sum).tobytes() == _vals(want.partial_sum).tobytes(), kind
    assert floats.walking_order == want_floats.walking_order and len(floats.walking_order) > 1
    for k in floats.walking_order:
        assert np.asarray(floats._weights[k], dtype=np.float64).tobytes() == np.asarray(want_floats._weights[k], dtype=np.float64).tobytes(), (kind, k)
    for g, r in zip(*(rng, other) if isinstance(rng, list) else ([rng], [other])):
        assert g.bit_generator.state == r.bit_generator.state
        assert np.array_equal(g.random(5), r.random(5))


def test_what_keeps_the_buffer(monkeypatch):
    monkeypatch.delenv("FLASHE_DEVICE_RNG", raising=False)
    monkeypatch.setenv("FLASHE_INLINE_DRAWS", "1")
    models = _host_models(C, SIZES, 12)
    # inline_draws=True and the default cohort, as before
    up, _f = _round(_cohort(128, False, False, inline_draws=True), models, np.random.default_rng(1), None)
    assert up.draws == "buffer"
    up, _f = _round(_cohort(20, False, True), models, np.random.default_rng(1), None)
    assert up.draws == "buffer"
    # a batched job: the launch has no batched form
    up, _f = _round(_cohort(120, True, False, inline_draws="any"), models, np.random.default_rng(1), None)
    assert up.draws == "buffer"
    # a list of PCG64 and Philox generators; of PCG64 and PCG64DXSM generators
    gens = [np.random.default_rng(c) for c in range(C - 1)] + [np.random.Generator(np.random.Philox(2))]
    up, _f = _round(_cohort(20, False, True, inline_draws="any"), models, gens, None)
    assert up.draws == "buffer"
    gens = [np.random.default_rng(c) for c in range(C - 1)] + [np.random.Generator(np.random.PCG64DXSM(2))]
    up, _f = _round(_cohort(128, False, False, inline_draws="any"), models, gens, None)
    assert up.draws == "buffer"
    # "any" does everything True does: Philox generators draw inline
    up, _f = _round(_cohort(128, False, False, inline_draws="any"), models, np.random.Generator(np.random.Philox(7)), None)
    assert up.draws == "inline"


@pytest.mark.parametrize("b,compact", [(128, False), (20, True)])
def test_unset_follows_the_default_table(monkeypatch, b, compact):
    from flashe_amd import block
    monkeypatch.delenv("FLASHE_DEVICE_RNG", raising=False)
    monkeypatch.delenv("FLASHE_INLINE_DRAWS", raising=False)
    models = _host_models(C, SIZES, 13)
    up, _f = _round(_cohort(b, False, compact, inline_draws="any"), models, np.random.default_rng(1), None)
    assert up.draws == ("inline" if block._INLINE_PCG64_DEFAULT[compact] else "buffer")
