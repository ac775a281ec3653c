"""CPU test: when does a "prepared-cohort" round generate its Philox draws inside the online launch (flashe_amd.block._inline_draws)?
The conditions -- un-batched, every generator over np.random.Philox, an engine with the call, FLASHE_DEVICE_RNG not 0 --, the A/B switch
FLASHE_INLINE_DRAWS (0 never, 1 always, unset: the default of the shape class), and the class of a round (_draws_aligned)."""
import numpy as np
import pytest

from flashe_amd import block


class _Eng:
    PHILOX_MAX_SEGMENTS = 128

    def quantize_combine_cohort_philox_dev(self, *a, **kw):
        raise AssertionError("not called here")


def _philox(pre=0):
    g = np.random.Generator(np.random.Philox(1))
    if pre:
        g.random(pre)
    return g


def test_alignment_of_a_round():
    assert block._draws_aligned(_philox(), 10, 1000) and block._draws_aligned(_philox(4), 10, 1000)
    assert not block._draws_aligned(_philox(), 10, 1001) and block._draws_aligned(_philox(), 1, 1001)
    assert not block._draws_aligned(_philox(1), 10, 1000)
    assert block._draws_aligned([_philox(), _philox(8)], 2, 1001)
    assert not block._draws_aligned([_philox(), _philox(3)], 2, 1000)


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("aligned", [False, True])
def test_the_switch_and_the_class_defaults(monkeypatch, compact, aligned):
    eng, rng, n = _Eng(), _philox(), 1000 if aligned else 1001
    monkeypatch.delenv("FLASHE_DEVICE_RNG", raising=False)
    monkeypatch.delenv("FLASHE_INLINE_DRAWS", raising=False)
    assert block._inline_draws(eng, rng, False, compact, 10, n) is block._INLINE_DRAWS_DEFAULT[(compact, aligned)]
    monkeypatch.setenv("FLASHE_INLINE_DRAWS", "1")
    assert block._inline_draws(eng, rng, False, compact, 10, n) is True
    assert block._inline_draws(eng, rng, True, compact, 10, n) is False                       # a batched job
    assert block._inline_draws(eng, np.random.default_rng(1), False, compact, 10, n) is False
    assert block._inline_draws(eng, [rng, np.random.default_rng(1)], False, compact, 2, n) is False
    assert block._inline_draws(eng, None, False, compact, 10, n) is False
    assert block._inline_draws(object(), rng, False, compact, 10, n) is False                 # an engine without the entry point
    assert block._inline_draws(eng, [rng] * 129, False, compact, 129, n) is False             # more generators than a table holds
    monkeypatch.setenv("FLASHE_DEVICE_RNG", "0")
    assert block._inline_draws(eng, rng, False, compact, 10, n) is False
    monkeypatch.delenv("FLASHE_DEVICE_RNG")
    monkeypatch.setenv("FLASHE_INLINE_DRAWS", "0")
    assert block._inline_draws(eng, rng, False, compact, 10, n) is False
