"""CPU-only: the host entry point that states the PCG64 / PCG64DXSM streams (flashe_pcg64_advance: the state n steps on, n below 2^128)
against NumPy's own bit generators -- bit_generator.state after Generator.random(n) from generators taken after 0 .. 3 draws and after a
32-bit draw, at states and increments set by hand to 0, 2^128 - 1 and an even value, and at far distances (2^32 +- 1, 2^64 +- 1, 2^127:
what no few-second device run reaches; the device launch compiles the same functions) against bit_generator.advance(k); a state set by
hand from the advance's output continues NumPy's stream with has_uint32 / uinteger as they were; then the segment table
Engine.pcg64_random_dev builds on that advance, without a device (draw_table_cases.py).  Touches no device."""
import ctypes

import numpy as np
import pytest

import draw_table_cases as cases
from flashe_amd import _lib
from flashe_amd.engine import _Pcg64Draws

U64 = ctypes.c_uint64
M64 = 2 ** 64 - 1
M128 = 2 ** 128 - 1
VARIANTS = {"PCG64": 0, "PCG64DXSM": 1}
HAND = [(0, 1), (M128, M128), (0x0123456789ABCDEFFEDCBA9876543210, 2), (12345, 0), (M128, 2 ** 64), (0, M128)]      # (state, inc)


def _words(v):
    return (U64 * 2)(v & M64, v >> 64)


def _advance(name, state, inc, n):
    s = _words(state)
    assert _lib.load().flashe_pcg64_advance(VARIANTS[name], s, _words(inc), _words(n)) == 0
    return int(s[0]) | (int(s[1]) << 64)


def _gen(name, seed=7, hand=None):
    g = np.random.Generator(getattr(np.random, name)(seed))
    if hand is not None:
        st = g.bit_generator.state
        st["state"]["state"], st["state"]["inc"] = hand
        g.bit_generator.state = st
    return g


@pytest.mark.parametrize("name", list(VARIANTS))
@pytest.mark.parametrize("pre", [0, 1, 2, 3])
def test_the_advance_is_numpys_state_after_n_draws(name, pre):
    for n in (0, 1, 2, 3, 255, 256, 257, 4096, 1000003):
        g = _gen(name)
        g.random(pre)
        start = g.bit_generator.state["state"]
        g.random(n)
        assert _advance(name, start["state"], start["inc"], n) == g.bit_generator.state["state"]["state"], (pre, n)


@pytest.mark.parametrize("name", list(VARIANTS))
@pytest.mark.parametrize("hand", HAND)
def test_states_and_increments_set_by_hand(name, hand):
    for n in (1, 2, 1025):
        g = _gen(name, hand=hand)
        assert (g.bit_generator.state["state"]["state"], g.bit_generator.state["state"]["inc"]) == hand       # NumPy takes them as they are
        g.random(n)
        assert _advance(name, hand[0], hand[1], n) == g.bit_generator.state["state"]["state"], (hand, n)


@pytest.mark.parametrize("name", list(VARIANTS))
@pytest.mark.parametrize("k", [2 ** 32 - 1, 2 ** 32 + 1, 2 ** 64 - 1, 2 ** 64 + 1, 2 ** 127])
def test_far_distances_against_numpys_own_advance(name, k):
    for hand in [None] + HAND:
        g = _gen(name, hand=hand)
        g.random(3)
        start = g.bit_generator.state["state"]
        g.bit_generator.advance(k)
        assert _advance(name, start["state"], start["inc"], k) == g.bit_generator.state["state"]["state"], (hand, k)
    # jump(a + b) = jump(b) o jump(a)
    s, inc = 0xDEADBEEF << 70, 0x1234567
    assert _advance(name, _advance(name, s, inc, k), inc, 5) == _advance(name, s, inc, (k + 5) & M128)


@pytest.mark.parametrize("name", list(VARIANTS))
def test_a_state_set_by_hand_from_the_advance_continues_the_stream_and_keeps_the_cached_word(name):
    for pre, n in ((0, 5), (2, 1), (3, 4097), (1, 1000003)):
        ref = _gen(name)
        ref.random(pre)
        ref.integers(0, 2 ** 32, dtype=np.uint32)                   # leaves has_uint32 = 1 and the other half of the word in uinteger
        start = ref.bit_generator.state
        assert start["has_uint32"] == 1
        ref.random(n)
        after = ref.bit_generator.state
        assert (after["has_uint32"], after["uinteger"]) == (1, start["uinteger"])      # random() neither reads nor changes them
        want = (ref.integers(0, 2 ** 32, 3, dtype=np.uint32).tobytes(), ref.random(9).tobytes())
        g = _gen(name, seed=99)                                     # another stream altogether
        state = g.bit_generator.state
        state["state"]["state"] = _advance(name, start["state"]["state"], start["state"]["inc"], n)
        state["state"]["inc"] = start["state"]["inc"]
        state["has_uint32"], state["uinteger"] = start["has_uint32"], start["uinteger"]
        g.bit_generator.state = state
        assert (g.integers(0, 2 ** 32, 3, dtype=np.uint32).tobytes(), g.random(9).tobytes()) == want, (pre, n)


def test_the_advance_refuses_a_bad_call():
    lib = _lib.load()
    s = _words(5)
    assert lib.flashe_pcg64_advance(2, s, _words(1), _words(1)) != 0
    assert lib.flashe_pcg64_advance(0, None, _words(1), _words(1)) != 0
    assert list(s) == [5, 0]


# ---- the segment table Engine.pcg64_random_dev builds on that advance (draw_table_cases.py: the checks, shared with Philox) ----
NAMES = {"PCG64": ["PCG64", "PCG64DXSM", "PCG64"], "PCG64DXSM": ["PCG64DXSM", "PCG64", "PCG64DXSM"]}    # both variants in every table


@pytest.mark.parametrize("name", list(VARIANTS))
@pytest.mark.parametrize("offsets", [cases.OFFSETS, None])
def test_the_draw_table_hands_back_the_states_of_the_same_host_draws(name, offsets):
    cases.handed_back_states_are_those_of_the_same_host_draws_in_list_order(_Pcg64Draws, NAMES[name], offsets)


@pytest.mark.parametrize("name", list(VARIANTS))
def test_the_draw_table_continues_a_repeated_entry(name):
    cases.a_repeated_entry_starts_where_its_earlier_segment_ends(_Pcg64Draws, NAMES[name])


@pytest.mark.parametrize("bad", cases.OUTSIDE_64_BITS)
@pytest.mark.parametrize("name", list(VARIANTS))
def test_the_draw_table_refuses_counts_and_offsets_outside_64_bits(name, bad):
    cases.counts_and_offsets_outside_64_bits_are_refused_with_nothing_advanced(_Pcg64Draws, NAMES[name], bad)


@pytest.mark.parametrize("name", list(VARIANTS))
def test_the_draw_table_refusals_advance_nothing(name):
    cases.the_other_refusals_advance_nothing(_Pcg64Draws, NAMES[name], [np.random.SFC64(1), np.random.MT19937(1), np.random.Philox(1)])
