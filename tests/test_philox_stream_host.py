"""CPU-only: the host entry points that state the Philox stream (flashe_philox_block: one Philox4x64-10 block; flashe_philox_advance: the
state after n draws) against NumPy's own np.random.Philox -- its first block for several keys and counters, Generator.bit_generator.state
after g.random(n) from generators pre-advanced by 0 .. 4 draws (buffer_pos 4, 1, 2, 3, 4), counters whose increment carries or wraps at
2^256, and a state set by hand from the advance's output that continues NumPy's stream; then the segment table Engine.philox_random_dev
builds on that advance, without a device (draw_table_cases.py).  Touches no device."""
import ctypes

import numpy as np
import pytest

import draw_table_cases as cases
from flashe_amd import _lib
from flashe_amd.engine import _PhiloxDraws

U64 = ctypes.c_uint64
M64 = 2 ** 64 - 1
KEYS = [(0, 0), (1, 2), (0x0123456789ABCDEF, M64)]
COUNTERS = [(0, 0, 0, 0), (7, 0, 0, 1), (M64 - 1, M64, 5, 0), (M64, M64, M64, M64)]


def _gen(key, counter):
    return np.random.Generator(np.random.Philox(key=np.array(key, dtype=np.uint64), counter=np.array(counter, dtype=np.uint64)))


def _block(counter, key):
    out = (U64 * 4)()
    assert _lib.load().flashe_philox_block((U64 * 4)(*counter), (U64 * 2)(*key), out) == 0
    return [int(v) for v in out]


def _advance(state, n):
    """(counter, buffer_pos, buffer) of flashe_philox_advance from a bit_generator.state."""
    key = (U64 * 2)(*[int(v) for v in state["state"]["key"]])
    counter = (U64 * 4)(*[int(v) for v in state["state"]["counter"]])
    buffer = (U64 * 4)(*[int(v) for v in state["buffer"]])
    pos = ctypes.c_uint32(int(state["buffer_pos"]))
    assert _lib.load().flashe_philox_advance(key, counter, ctypes.byref(pos), buffer, n) == 0
    return [int(v) for v in counter], int(pos.value), [int(v) for v in buffer]


def _triple(state):
    return [int(v) for v in state["state"]["counter"]], int(state["buffer_pos"]), [int(v) for v in state["buffer"]]


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("counter", COUNTERS)
def test_the_block_is_numpys_first_block(key, counter):
    g = _gen(key, counter)
    first = g.bit_generator.random_raw(4)                           # NumPy increments the counter, then generates
    inc = [int(v) for v in g.bit_generator.state["state"]["counter"]]
    total = (sum(c << (64 * i) for i, c in enumerate(counter)) + 1) % (1 << 256)
    assert inc == [(total >> (64 * i)) & M64 for i in range(4)]
    assert _block(inc, key) == [int(v) for v in first]
    assert _block(inc, key) == [int(v) for v in g.bit_generator.state["buffer"]]


@pytest.mark.parametrize("counter", COUNTERS)
@pytest.mark.parametrize("pre", [0, 1, 2, 3, 4])
def test_the_advance_is_numpys_state_after_n_draws(counter, pre):
    key = KEYS[2]
    for n in (0, 1, 3, 4, 5, 8, 1000003):
        g = _gen(key, counter)
        g.random(pre)
        start = g.bit_generator.state
        assert start["buffer_pos"] == (4 if pre == 0 else (pre - 1) % 4 + 1)
        g.random(n)
        assert _advance(start, n) == _triple(g.bit_generator.state), (pre, n)


@pytest.mark.parametrize("counter", COUNTERS)
def test_a_state_set_by_hand_from_the_advance_continues_the_stream(counter):
    key = KEYS[1]
    for pre, n in ((0, 5), (2, 1), (3, 6), (4, 4), (1, 1000003)):
        ref = _gen(key, counter)
        ref.random(pre)
        start = ref.bit_generator.state
        ref.random(n)
        want = ref.random(9)
        g = _gen((5, 5), (9, 9, 9, 9))                                # another stream altogether
        state = g.bit_generator.state
        c, p, b = _advance(start, n)
        state["state"]["key"] = np.array(key, dtype=np.uint64)
        state["state"]["counter"] = np.array(c, dtype=np.uint64)
        state["buffer"], state["buffer_pos"] = np.array(b, dtype=np.uint64), p
        g.bit_generator.state = state
        assert g.random(9).tobytes() == want.tobytes(), (pre, n)


def test_the_advance_refuses_a_bad_state():
    lib = _lib.load()
    key, counter, buffer = (U64 * 2)(), (U64 * 4)(), (U64 * 4)()
    assert lib.flashe_philox_advance(key, counter, ctypes.byref(ctypes.c_uint32(5)), buffer, 1) != 0
    assert lib.flashe_philox_advance(key, counter, ctypes.byref(ctypes.c_uint32(4)), buffer, 2 ** 60 + 1) != 0
    assert list(counter) == [0, 0, 0, 0]


# ---- the segment table Engine.philox_random_dev builds on that advance (draw_table_cases.py: the checks, shared with the PCG64 kinds) ----
NAMES = ["Philox"] * 3


@pytest.mark.parametrize("offsets", [cases.OFFSETS, None])
def test_the_draw_table_hands_back_the_states_of_the_same_host_draws(offsets):
    cases.handed_back_states_are_those_of_the_same_host_draws_in_list_order(_PhiloxDraws, NAMES, offsets)


def test_the_draw_table_continues_a_repeated_entry():
    cases.a_repeated_entry_starts_where_its_earlier_segment_ends(_PhiloxDraws, NAMES)


@pytest.mark.parametrize("bad", cases.OUTSIDE_64_BITS)
def test_the_draw_table_refuses_counts_and_offsets_outside_64_bits(bad):
    cases.counts_and_offsets_outside_64_bits_are_refused_with_nothing_advanced(_PhiloxDraws, NAMES, bad)


def test_the_draw_table_refusals_advance_nothing():
    cases.the_other_refusals_advance_nothing(_PhiloxDraws, NAMES, [np.random.SFC64(1), np.random.MT19937(1), np.random.PCG64(1)])
