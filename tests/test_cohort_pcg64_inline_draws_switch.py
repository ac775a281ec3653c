"""CPU test: when does a "prepared-cohort" round generate its PCG64 / PCG64DXSM draws inside the online launch
(flashe_amd.block._inline_pcg64_draws, asked by FlasheCohort(inline_draws="any"))?  The conditions -- un-batched, every generator of ONE of
the two variants, at most PCG64_MAX_SEGMENTS of them, an engine with the call, FLASHE_DEVICE_RNG not 0 --, the A/B switch
FLASHE_INLINE_DRAWS (0 never, 1 always, unset: the layout's default in _INLINE_PCG64_DEFAULT); what inline_draws=True asks is unchanged
(_inline_draws never takes a PCG64 generator); and the cohort's routing of a round to the engine's call, on a stub engine."""
import numpy as np
import pytest

from flashe_amd import block


class _Eng:
    PHILOX_MAX_SEGMENTS = 128
    PCG64_MAX_SEGMENTS = 128

    def quantize_combine_cohort_philox_dev(self, *a, **kw):
        raise AssertionError("not called here")

    def quantize_combine_cohort_pcg64_dev(self, *a, **kw):
        raise AssertionError("not called here")


class _OldEng:
    PHILOX_MAX_SEGMENTS = 128
    PCG64_MAX_SEGMENTS = 128

    def quantize_combine_cohort_philox_dev(self, *a, **kw):
        raise AssertionError("not called here")


def _dxsm(seed=1):
    return np.random.Generator(np.random.PCG64DXSM(seed))


def _philox(seed=1):
    return np.random.Generator(np.random.Philox(seed))


@pytest.mark.parametrize("compact", [False, True])
def test_the_switch_and_the_layout_defaults(monkeypatch, compact):
    eng, rng = _Eng(), np.random.default_rng(1)
    monkeypatch.delenv("FLASHE_DEVICE_RNG", raising=False)
    monkeypatch.delenv("FLASHE_INLINE_DRAWS", raising=False)
    assert set(block._INLINE_PCG64_DEFAULT) == {False, True}
    assert block._inline_pcg64_draws(eng, rng, False, compact) is block._INLINE_PCG64_DEFAULT[compact]
    for value in (False, True):                                                      # unset follows the table, whatever it holds
        monkeypatch.setitem(block._INLINE_PCG64_DEFAULT, compact, value)
        assert block._inline_pcg64_draws(eng, rng, False, compact) is value
        assert block._inline_pcg64_draws(eng, [_dxsm(1), _dxsm(2)], False, compact) is value
    monkeypatch.setenv("FLASHE_INLINE_DRAWS", "1")
    monkeypatch.setitem(block._INLINE_PCG64_DEFAULT, compact, False)
    assert block._inline_pcg64_draws(eng, rng, False, compact) is True
    assert block._inline_pcg64_draws(eng, _dxsm(), False, compact) is True
    assert block._inline_pcg64_draws(eng, [np.random.default_rng(c) for c in range(128)], False, compact) is True
    assert block._inline_pcg64_draws(eng, [rng, rng, rng], False, compact) is True                # the same Generator three times
    assert block._inline_pcg64_draws(eng, rng, True, compact) is False                             # a batched job
    assert block._inline_pcg64_draws(eng, [rng, _dxsm()], False, compact) is False                 # both variants in one list
    assert block._inline_pcg64_draws(eng, [rng, _philox()], False, compact) is False               # a mixed list
    assert block._inline_pcg64_draws(eng, _philox(), False, compact) is False
    assert block._inline_pcg64_draws(eng, np.random.Generator(np.random.SFC64(1)), False, compact) is False
    assert block._inline_pcg64_draws(eng, None, False, compact) is False
    assert block._inline_pcg64_draws(_OldEng(), rng, False, compact) is False                      # an engine without the call
    assert block._inline_pcg64_draws(eng, [np.random.default_rng(c) for c in range(129)], False, compact) is False
    monkeypatch.setenv("FLASHE_DEVICE_RNG", "0")
    assert block._inline_pcg64_draws(eng, rng, False, compact) is False
    monkeypatch.delenv("FLASHE_DEVICE_RNG")
    monkeypatch.setenv("FLASHE_INLINE_DRAWS", "0")
    monkeypatch.setitem(block._INLINE_PCG64_DEFAULT, compact, True)
    assert block._inline_pcg64_draws(eng, rng, False, compact) is False


def test_what_inline_draws_true_asks_is_unchanged(monkeypatch):
    """_inline_draws, the rule of inline_draws=False and True, takes no PCG64 generator whatever the switch says."""
    monkeypatch.delenv("FLASHE_DEVICE_RNG", raising=False)
    monkeypatch.setenv("FLASHE_INLINE_DRAWS", "1")
    for rng in (np.random.default_rng(1), _dxsm(), [np.random.default_rng(1), np.random.default_rng(2)]):
        assert block._inline_draws(_Eng(), rng, False, False, 2, 1000) is False
        assert block._inline_draws(_Eng(), rng, True, False, 2, 1000, inline_batched=True, bs=6) is False
    assert block._inline_draws(_Eng(), _philox(), False, False, 2, 1000) is True


def test_the_keyword_takes_any_and_no_other_string():
    """validated before anything else of the cohort is built"""
    with pytest.raises(ValueError, match="inline_draws"):
        block.FlasheCohort({}, 0, 2, 4, 1, inline_draws="all")
    with pytest.raises(ValueError, match="inline_draws"):
        block.FlasheCohort({}, 0, 2, 4, 1, inline_draws="")


class _Plan:
    present, n, n_elems = [0, 1, 3], 1001, 1001


class _Buf:
    def __init__(self, name):
        self.buf = name


def test_the_cohort_hands_the_round_to_the_pcg64_call():
    """_launch_prepared_inline(pcg64=True): one shared generator is ONE entry of C n draws, a list one entry per present client; the compact
    flag and the masks of the present clients go along; the Philox call is not asked."""
    calls = []

    class _Engine(_Eng):
        def quantize_combine_cohort_pcg64_dev(self, n, rows, srcs, dts, bits, gens, counts, offsets, masks, cts, sum_out, compact=False):
            calls.append((n, bits, gens, counts, offsets, masks, cts, sum_out, compact))
            return True

    co = block.FlasheCohort.__new__(block.FlasheCohort)
    co.compact = True
    co._masks = [_Buf(f"m{p}") for p in range(4)]

    class _Lead:
        batch = False

        class quantizer:
            element_bits, num_clients = 16, 4

        class cipher:
            engine = _Engine()
    co.lead = _Lead()
    shared, cts, psum = np.random.default_rng(3), [_Buf("c0"), _Buf("c1"), _Buf("c2")], _Buf("s")
    assert co._launch_prepared_inline(_Plan(), "rows", "srcs", "dts", shared, cts, psum, True) is True
    assert calls[-1] == (1001, 16, [shared], [3003], [0], ["m0", "m1", "m3"], ["c0", "c1", "c2"], "s", True)
    each = [np.random.default_rng(c) for c in range(3)]
    assert co._launch_prepared_inline(_Plan(), "rows", "srcs", "dts", each, cts, psum, pcg64=True) is True
    assert calls[-1][2:5] == (each, [1001] * 3, [0, 1001, 2002])
