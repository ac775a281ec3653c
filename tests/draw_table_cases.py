"""The checks of the segment table Engine.philox_random_dev and Engine.pcg64_random_dev hand to their C calls (engine._draw_table, one body
for both kinds), built without a device; test_philox_stream_host.py and test_pcg64_stream_host.py run them for their kind.  A list in
which one Generator appears twice with another between, an empty segment, explicit offsets and a state dict in place of a Generator; then
every segment is advanced by its count with the kind's host advance entry point, which is what the device call does to the table, and the
states handed back must be those of NumPy generators that made the same random(n) calls in list order -- a cached 32-bit word
(has_uint32 = 1) included.  Counts and offsets outside 64 bits, which ctypes would mask silently, and the other refusals raise with
nothing advanced.  `names`: the bit generators of the three generators of a case."""
import numpy as np
import pytest

from flashe_amd._lib import FlasheError
from flashe_amd.engine import _draw_table

COUNTS = [1030, 17, 0, 2051, 9, 70]                 # entries g, h, h, g, state dict of d, g
OFFSETS = [4, 5000, 1, 1034, 3085, 2 ** 60 - 70]
OUTSIDE_64_BITS = [-1, 2 ** 64, 2 ** 64 + 4]


def _gens(names):
    """Three generators of the named bit generators: after 3 host draws, after a 32-bit draw (which leaves has_uint32 = 1), fresh."""
    g, h, d = [np.random.Generator(getattr(np.random, name)(seed)) for seed, name in zip((8, 3, 5), names)]
    g.random(3)
    h.integers(0, 2 ** 32, dtype=np.uint32)
    assert h.bit_generator.state["has_uint32"] == 1
    return g, h, d


def _same_state(a, b):
    """Two bit_generator.state dicts, arrays included."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same_state(a[k], b[k]) for k in a)
    return np.array_equal(a, b)


def handed_back_states_are_those_of_the_same_host_draws_in_list_order(kind, names, offsets):
    (g, h, d), refs = _gens(names), _gens(names)
    st = d.bit_generator.state
    segs, counts, offs, hand_back = _draw_table(kind, [g, h, h, g, st, g], COUNTS, offsets)
    for s in range(6):
        kind.move_on(segs[s], segs[s].n)                                             # as the C call advances the table
    hand_back()
    assert [int(segs[s].n) for s in range(6)] == COUNTS == counts
    assert offs == (OFFSETS if offsets is not None else [0, 1030, 1047, 1047, 3098, 3107]) and [int(segs[s].offset) for s in range(6)] == offs
    for ref, n in zip([refs[e] for e in (0, 1, 1, 0, 2, 0)], COUNTS):
        ref.random(n)
    for got, ref in zip((g, h), refs):
        assert _same_state(got.bit_generator.state, ref.bit_generator.state)          # has_uint32 / uinteger as they were
        assert got.integers(0, 2 ** 32, 3, dtype=np.uint32).tobytes() == ref.integers(0, 2 ** 32, 3, dtype=np.uint32).tobytes()
        assert got.random(7).tobytes() == ref.random(7).tobytes()
    assert _same_state(st, refs[2].bit_generator.state)                              # the dict moved,
    assert not _same_state(d.bit_generator.state, st) and d.random(2).tobytes() == _gens(names)[2].random(2).tobytes()    # its generator did not


def a_repeated_entry_starts_where_its_earlier_segment_ends(kind, names):
    (g, h, _d), (rg, _rh, _rd) = _gens(names), _gens(names)
    segs, _c, _o, _hand_back = _draw_table(kind, [g, h, g], [1030, 17, 5])

    def generator_fields(seg):
        vals = {f: getattr(seg, f) for f, _t in kind.Segment._fields_ if f not in ("n", "offset", "reserved")}
        return {f: list(v) if hasattr(v, "_length_") else v for f, v in vals.items()}

    assert generator_fields(segs[0]) == generator_fields(kind.segment(rg.bit_generator.state))
    rg.random(1030)
    assert generator_fields(segs[2]) == generator_fields(kind.segment(rg.bit_generator.state))
    assert (segs[2].n, segs[2].offset) == (5, 1047)


def counts_and_offsets_outside_64_bits_are_refused_with_nothing_advanced(kind, names, bad):
    (g, h, d), refs = _gens(names), _gens(names)
    st = d.bit_generator.state
    with pytest.raises(FlasheError):
        _draw_table(kind, [g, h, g, st], [4, 4, bad, 4])
    with pytest.raises(FlasheError):
        _draw_table(kind, [g, h, g, st], [4, 4, 4, 4], offsets=[0, 4, 8, bad])
    with pytest.raises(FlasheError):
        _draw_table(kind, [g], [bad])
    for got, ref in zip((g, h, d), refs):
        assert _same_state(got.bit_generator.state, ref.bit_generator.state)
    assert _same_state(st, refs[2].bit_generator.state)


def the_other_refusals_advance_nothing(kind, names, others):
    """others: bit generators that are not of the kind."""
    (g, h, _d), refs = _gens(names), _gens(names)
    with pytest.raises(ValueError):
        _draw_table(kind, [g, h], [4])
    with pytest.raises(ValueError):
        _draw_table(kind, [g, h], [4, 4], offsets=[0])
    with pytest.raises(ValueError):
        _draw_table(kind, [g] * (kind.max_segments + 1), [0] * (kind.max_segments + 1))
    for other in others:
        with pytest.raises(FlasheError):
            _draw_table(kind, [g, g, np.random.Generator(other)], [4, 4, 4])
    _draw_table(kind, [g] * kind.max_segments, [1] * kind.max_segments)                # a table that is built and never drawn
    for got, ref in zip((g, h), refs):
        assert _same_state(got.bit_generator.state, ref.bit_generator.state)
