"""GPU, class level: a BATCHED precompute job's FlasheCohort(inline_draws=True) whose rng= generators are over np.random.Philox draws
INSIDE its online launch (CohortUpload.draws == "inline": no draw buffer) -- every ciphertext, the sum, decrypt_unquantize's floats and
the generators' final states against a second identical cohort run with FLASHE_INLINE_DRAWS=0 ("buffer").  int_bits 120 (six values per
element) and 128 with element_bits 14 (seven).  The rounds from ONE shared generator (all clients, and present=) are in a listed class
of _INLINE_BATCHED_DEFAULT and run with FLASHE_INLINE_DRAWS unset: quantize_encrypt's own choice must say "inline".  The round from a
list of generators is not a listed class: unset it says "buffer", and it is compared under FLASHE_INLINE_DRAWS=1.  Without the keyword,
and with another bit generator, the round keeps the buffer."""
import copy

import numpy as np
import pytest

from test_gpu_cohort import KEY, _W, _host_models
from test_gpu_cohort_prepared_class import IT, SIZES, _args, _n_ct, _vals
from test_gpu_cohort_prepared_philox import _state_equal
from test_gpu_cohort_prepared_philox_class import _rngs, _round

pytestmark = pytest.mark.gpu

C = 10


def _cohort(b, **kw):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheCohort
    cm.N_JOBS = 16
    args = _args(b, True, _n_ct(SIZES, b, True, C))
    if b == 128:                                                      # fields of 14 + 4 bits: seven values per element
        args["quantize"]["element_bits"] = 14
        args["precompute"]["num_params"] = sum((s + 6) // 7 for s in SIZES)
    co = FlasheCohort(args, first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, **kw)
    co.set_iter_index(IT - 1)
    co.prepare_encrypt()
    co.set_iter_index(IT)
    return co


@pytest.mark.parametrize("kind", ["one", "list", "present"])
@pytest.mark.parametrize("b", [120, 128])
def test_a_batched_rounds_inline_draws_are_the_buffer_forms_bytes(monkeypatch, b, kind):
    from flashe_amd import block
    models = _host_models(C, SIZES, 11)
    rng, present = _rngs(kind)
    other = copy.deepcopy(rng)
    monkeypatch.delenv("FLASHE_DEVICE_RNG", raising=False)
    monkeypatch.delenv("FLASHE_INLINE_DRAWS", raising=False)
    co = _cohort(b, inline_draws=True)
    q = co.lead.quantizer
    bs = b // block._field_bits(q.element_bits, q.num_clients)
    assert bs == {120: 6, 128: 7}[b]
    n_clients = C if present is None else len(present)
    # the round's class, from the round's own arguments: one shared generator at an odd position is listed, a list is not
    listed = block._INLINE_BATCHED_DEFAULT.get(block._batched_draws_class(rng, bs, n_clients, sum(SIZES)), False)
    assert listed is (kind != "list")
    if not listed:
        monkeypatch.setenv("FLASHE_INLINE_DRAWS", "1")
    up, floats = _round(co, models, rng, present)
    assert up.path == "prepared-cohort" and up.draws == "inline"
    monkeypatch.setenv("FLASHE_INLINE_DRAWS", "0")
    want, want_floats = _round(_cohort(b, inline_draws=True), models, other, present)
    assert want.path == "prepared-cohort" and want.draws == "buffer"
    assert up.present == want.present and len(up.ciphertexts) == len(want.ciphertexts) == n_clients
    for c in range(len(want.ciphertexts)):
        assert _vals(up.ciphertexts[c]).tobytes() == _vals(want.ciphertexts[c]).tobytes(), (kind, c)
    assert _vals(up.partial_sum).tobytes() == _vals(want.partial_sum).tobytes(), kind
    assert floats.walking_order == want_floats.walking_order and len(floats.walking_order) > 1
    for k in floats.walking_order:
        assert np.asarray(floats._weights[k], dtype=np.float64).tobytes() == np.asarray(want_floats._weights[k], dtype=np.float64).tobytes(), (kind, k)
    for g, r in zip(*(rng, other) if isinstance(rng, list) else ([rng], [other])):
        assert _state_equal(g, r)
        assert np.array_equal(g.random(5), r.random(5))


def test_the_rounds_own_choice_without_the_switch(monkeypatch):
    """FLASHE_INLINE_DRAWS unset: the keyword and a shared Philox generator at an odd position say "inline"; without the keyword,
    with a block-aligned shared generator or a list of generators (not listed classes) and with default_rng the round says "buffer"."""
    monkeypatch.delenv("FLASHE_DEVICE_RNG", raising=False)
    monkeypatch.delenv("FLASHE_INLINE_DRAWS", raising=False)
    models = _host_models(C, SIZES, 12)
    def odd():
        g = np.random.Generator(np.random.Philox(7))
        g.random(3)
        return g

    for b in (120, 128):
        up, _f = _round(_cohort(b, inline_draws=True), models, odd(), None)
        assert up.draws == "inline", b
    up, _f = _round(_cohort(120), models, odd(), None)
    assert up.draws == "buffer"
    # a fresh shared generator over 30,000 values: every client starts at a block -- not a listed class
    assert sum(SIZES) % 4 == 0
    up, _f = _round(_cohort(120, inline_draws=True), models, np.random.Generator(np.random.Philox(7)), None)
    assert up.draws == "buffer"
    up, _f = _round(_cohort(120, inline_draws=True), models, [np.random.Generator(np.random.Philox(7 + c)) for c in range(C)], None)
    assert up.draws == "buffer"
    up, _f = _round(_cohort(120, inline_draws=True), models, np.random.default_rng(1), None)
    assert up.draws == "buffer"


def test_the_switch_forces_the_form_only_where_the_keyword_asked(monkeypatch):
    monkeypatch.delenv("FLASHE_DEVICE_RNG", raising=False)
    monkeypatch.setenv("FLASHE_INLINE_DRAWS", "1")
    models = _host_models(C, SIZES, 12)
    up, _f = _round(_cohort(120), models, np.random.Generator(np.random.Philox(7)), None)
    assert up.draws == "buffer"
    up, _f = _round(_cohort(120, inline_draws=True), models, np.random.default_rng(1), None)
    assert up.draws == "buffer"
    up, _f = _round(_cohort(120, inline_draws=True), models, [np.random.Generator(np.random.Philox(7 + c)) for c in range(C)], None)
    assert up.draws == "inline"
