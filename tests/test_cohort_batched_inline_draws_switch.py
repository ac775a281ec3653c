"""CPU test: when does a BATCHED "prepared-cohort" round generate its Philox draws inside the online launch
(flashe_amd.block._inline_draws with inline_batched=, FlasheCohort(inline_draws=True))?  Keyword off: never.  Keyword on: the class
table _INLINE_BATCHED_DEFAULT; FLASHE_INLINE_DRAWS=1: always; FLASHE_INLINE_DRAWS=0 or FLASHE_DEVICE_RNG=0: never; another bit
generator or more generators than a table holds: never; an engine without the batched call: never."""
import numpy as np
import pytest

from flashe_amd import block


class _Eng:
    """an engine double that has both calls"""
    PHILOX_MAX_SEGMENTS = 128

    def quantize_combine_cohort_philox_dev(self, *a, **kw):
        raise AssertionError("not called here")

    def quantize_batch_combine_cohort_philox_dev(self, *a, **kw):
        raise AssertionError("not called here")


class _OldEng:
    PHILOX_MAX_SEGMENTS = 128

    def quantize_combine_cohort_philox_dev(self, *a, **kw):
        raise AssertionError("not called here")


def _philox(pre=0):
    g = np.random.Generator(np.random.Philox(1))
    if pre:
        g.random(pre)
    return g


@pytest.mark.parametrize("bs", [1, 3, 5, 6, 7, 9])
@pytest.mark.parametrize("aligned", [False, True])
def test_the_keyword_the_switch_and_the_class_table(monkeypatch, bs, aligned):
    eng, rng, n = _Eng(), _philox(), 1000 if aligned else 1001
    monkeypatch.delenv("FLASHE_DEVICE_RNG", raising=False)
    monkeypatch.delenv("FLASHE_INLINE_DRAWS", raising=False)
    ask = lambda e=eng, r=rng, C=10, **kw: block._inline_draws(e, r, True, False, C, n, bs=bs, **kw)       # noqa: E731
    assert ask() is False and ask(inline_batched=False) is False                                  # keyword off
    assert ask(inline_batched=True) is block._INLINE_BATCHED_DEFAULT.get((bs, True, aligned), False)     # keyword on: the class table
    assert ask(inline_batched=True) is (bs in (6, 7) and not aligned)                             # (what the measurement left in it)
    for gens in ([_philox(), _philox(4)], [_philox(1), _philox(3)]):                              # a list, aligned or not: not a listed class
        assert block._batched_draws_class(gens, bs, 2, n) == (bs, False, gens[0].bit_generator.state["buffer_pos"] == 4)
        assert ask(r=gens, C=2, inline_batched=True) is False
    monkeypatch.setenv("FLASHE_INLINE_DRAWS", "1")
    assert ask(inline_batched=True) is True
    assert ask() is False                                                                          # (forced, but not opted in)
    assert ask(r=np.random.default_rng(1), inline_batched=True) is False                           # PCG64
    assert ask(r=[rng, np.random.default_rng(1)], C=2, inline_batched=True) is False
    assert ask(r=[rng] * 129, C=129, inline_batched=True) is False                                 # more generators than a table holds
    assert ask(r=None, inline_batched=True) is False
    assert ask(e=_OldEng(), inline_batched=True) is False                                          # an engine without the batched call
    assert block._inline_draws(_OldEng(), rng, False, False, 10, n) is True                        # (its un-batched call is still taken)
    monkeypatch.setenv("FLASHE_DEVICE_RNG", "0")
    assert ask(inline_batched=True) is False
    monkeypatch.delenv("FLASHE_DEVICE_RNG")
    monkeypatch.setenv("FLASHE_INLINE_DRAWS", "0")
    assert ask(inline_batched=True) is False


def test_the_class_table_holds_measured_classes_only():
    """Keys are (compiled-in values per element, one shared generator?, aligned?) and only classes that won are listed."""
    for (bs, shared, aligned), on in block._INLINE_BATCHED_DEFAULT.items():
        assert bs in (5, 6, 7) and isinstance(shared, bool) and isinstance(aligned, bool) and on is True


def test_the_cohort_takes_the_keyword():
    import inspect
    from flashe_amd.block import FlasheCohort
    assert inspect.signature(FlasheCohort.__init__).parameters["inline_draws"].default is False
