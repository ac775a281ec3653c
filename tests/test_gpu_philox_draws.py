"""GPU: Engine.philox_random_dev (flashe_philox_random_dev: philox_random_args_kernel / philox_random_table_kernel) against
Generator(np.random.Philox(key=..., counter=...)).random(n), compared as bytes: the lengths around one block and around one tile, the
lengths either side of a workgroup's second trip through its loop (read from the launcher's grid rule on a ctx limited to one CU), start
states with buffer_pos 1, 2, 3 and 4, counters whose increment carries or wraps at 2^256, an output pointer 8 bytes past a 32-byte
boundary, several ragged segments in one launch, more segments than the kernel arguments hold, the same generator twice -- with canary
values either side of every range that must come back intact, and the host generator continuing NumPy's own stream afterwards -- a state
dict advanced in place, and the refusals (a count outside 64 bits and a call inside a graph capture among them), which advance and write
nothing."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M64 = 2 ** 64 - 1
KEY = bytes(range(32))
CANARY = -7.25
KEYS = [(0, 0), (0x0123456789ABCDEF, M64)]
COUNTERS = {"zero": (0, 0, 0, 0), "carry": (M64 - 1, M64, 5, 0), "wrap": (M64, M64, M64, M64)}


def _gen(key, counter, pre=0):
    g = np.random.Generator(np.random.Philox(key=np.array(key, dtype=np.uint64), counter=np.array(counter, dtype=np.uint64)))
    g.random(pre)                                   # buffer_pos 4, 1, 2, 3, 4 for pre = 0 .. 4
    return g


@pytest.fixture(scope="module")
def eng():
    from flashe_amd import Engine
    e = Engine(KEY, 64)
    e.set_cu_limit(1)                               # 8 workgroups: a second trip from 8 tiles (8,192 draws) on
    return e


def _check(eng, specs, lead=4, gap=3, shift=0, repeat=None):
    """specs: (key, counter, pre, n) per segment, laid out `gap` draws apart from draw `lead` of a canary-filled buffer whose address the call
    is given `shift` draws in.  Every range against NumPy, everything else untouched, and the generators continue NumPy's stream."""
    gens = [_gen(k, c, pre) for k, c, pre, _n in specs]
    refs = [_gen(k, c, pre) for k, c, pre, _n in specs]
    counts = [n for _k, _c, _pre, n in specs]
    if repeat is not None:                          # segment `repeat` draws from segment 0's generator, continuing it
        gens[repeat] = gens[0]
    offsets, at = [], lead
    for n in counts:
        offsets.append(at)
        at += n + gap
    total = shift + at + 5
    buf = eng.upload(np.full(total, CANARY))
    out = eng.philox_random_dev(gens, counts, out=buf.ptr + 8 * shift, offsets=offsets)
    assert out == buf.ptr + 8 * shift
    got = buf.download(np.float64, total)
    want = np.full(total, CANARY)
    for s, (off, n) in enumerate(zip(offsets, counts)):
        src = refs[0] if repeat is not None and s == repeat else refs[s]
        want[shift + off:shift + off + n] = src.random(n)
    assert got.tobytes() == want.tobytes(), (offsets, counts, np.flatnonzero(got != want)[:8])
    for s, (g, r) in enumerate(zip(gens, refs)):
        if repeat is not None and s == repeat:
            continue
        assert g.random(7).tobytes() == r.random(7).tobytes(), s
        a, b = g.bit_generator.state, r.bit_generator.state
        assert a["buffer_pos"] == b["buffer_pos"] and a["has_uint32"] == b["has_uint32"] and a["uinteger"] == b["uinteger"]
        assert np.array_equal(a["state"]["counter"], b["state"]["counter"]) and np.array_equal(a["buffer"], b["buffer"])


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 1023, 1024, 1025])
def test_lengths_around_a_block_and_a_tile_from_every_buffer_position(eng, n):
    for pre in range(5):
        _check(eng, [(KEYS[1], COUNTERS["zero"], pre, n)], lead=4)          # a 32-byte aligned range
        _check(eng, [(KEYS[1], COUNTERS["zero"], pre, n)], lead=1)          # 8 bytes past a 32-byte boundary
        _check(eng, [(KEYS[1], COUNTERS["zero"], pre, n)], lead=2, shift=1)


@pytest.mark.parametrize("pre", [0, 1, 2, 3])
def test_lengths_either_side_of_a_workgroups_second_trip(eng, pre):
    cap, _tiles = eng.philox_grid(1 << 30)
    assert cap == 8                                                         # (one CU: stream_grid's 8 workgroups per CU)
    skip = pre                                                              # buffer_pos = pre for pre 1 .. 3; a fresh buffer skips nothing
    n2 = cap * 1024 - skip + 1                                              # the first length whose blocks need tile cap + 1
    pos = 4 if pre == 0 else pre
    assert eng.philox_grid(n2 - 1, pos) == (cap, cap) and eng.philox_grid(n2, pos) == (cap, cap + 1)
    for n in (n2 - 1, n2, n2 + 1):
        _check(eng, [(KEYS[0], COUNTERS["carry"], pre, n)], lead=3)


@pytest.mark.parametrize("counter", list(COUNTERS))
@pytest.mark.parametrize("key", KEYS)
def test_counters_that_carry_and_wrap(eng, key, counter):
    for pre in (0, 1, 3):
        _check(eng, [(key, COUNTERS[counter], pre, 1029)], lead=5)


def test_several_ragged_segments_in_one_launch(eng):
    k, z = KEYS[1], COUNTERS["zero"]
    _check(eng, [(k, z, 0, 5), ((9, 9), COUNTERS["carry"], 2, 4099), (k, COUNTERS["wrap"], 3, 1)], lead=1, gap=0)     # back to back
    _check(eng, [(k, z, 0, 5), ((9, 9), COUNTERS["carry"], 2, 4099), (k, COUNTERS["wrap"], 3, 1)], lead=2, gap=1)
    _check(eng, [((1, 1), z, 1, 4097), ((2, 2), z, 0, 4097)], lead=0, gap=0)                                             # the K + 1 shape
    _check(eng, [((1, 1), z, 1, 4097), ((2, 2), z, 0, 4097)], lead=3, gap=0, shift=1)
    _check(eng, [(k, z, 0, 0), (k, z, 2, 9), (k, z, 4, 0)])                                                              # empty segments


def test_more_segments_than_the_kernel_arguments_hold(eng):
    specs = [((s, 7), COUNTERS["carry" if s % 3 == 0 else "zero"], s % 5, 1 + (37 * s) % 1500) for s in range(128)]
    _check(eng, specs, lead=1, gap=1)
    _check(eng, specs[:49], lead=2, gap=0)
    _check(eng, specs[:48], lead=2, gap=0)


def test_the_same_generator_twice_continues_itself(eng):
    k, z = KEYS[1], COUNTERS["zero"]
    _check(eng, [(k, z, 1, 1030), ((3, 3), z, 0, 17), (k, z, 1, 2051)], repeat=2)


def test_the_refusals_advance_nothing(eng):
    from flashe_amd._lib import FlasheError
    g, h = _gen(KEYS[0], COUNTERS["zero"], 2), _gen(KEYS[1], COUNTERS["zero"])
    buf = eng.upload(np.full(64, CANARY))
    before = (g.bit_generator.state, h.bit_generator.state)
    with pytest.raises(FlasheError):
        eng.philox_random_dev([g, h], [10, 10], out=buf, offsets=[0, 9])                     # overlapping ranges
    with pytest.raises(FlasheError):
        eng.philox_random_dev([g], [2 ** 60 + 1], out=buf)
    with pytest.raises(FlasheError):
        eng.philox_random_dev([g], [4], out=buf.ptr + 4)                                      # a misaligned output
    with pytest.raises(FlasheError):
        eng.philox_random_dev([np.random.Generator(np.random.PCG64(1))], [4], out=buf)
    with pytest.raises(ValueError):
        eng.philox_random_dev([g] * 129, [0] * 129, out=buf)
    bad = g.bit_generator.state
    bad["buffer_pos"] = 5
    with pytest.raises(FlasheError):
        eng.philox_random_dev([bad], [4], out=buf)
    eng.sync()
    assert buf.download(np.float64, 64).tobytes() == np.full(64, CANARY).tobytes()
    for gen, st in zip((g, h), before):
        now = gen.bit_generator.state
        assert now["buffer_pos"] == st["buffer_pos"] and np.array_equal(now["state"]["counter"], st["state"]["counter"])


def _unmoved(g, before):
    now = g.bit_generator.state
    return (now["buffer_pos"] == before["buffer_pos"] and np.array_equal(now["state"]["counter"], before["state"]["counter"])
            and np.array_equal(now["buffer"], before["buffer"]))


def test_a_count_or_offset_outside_64_bits_is_refused(eng):
    """(ctypes masks such a value silently: 2 ** 64 + 4 would draw 4 values and advance the generator by 4)"""
    from flashe_amd._lib import FlasheError
    g = _gen(KEYS[1], COUNTERS["zero"], 2)
    before = g.bit_generator.state
    buf = eng.upload(np.full(64, CANARY))
    with pytest.raises(FlasheError):
        eng.philox_random_dev([g], [2 ** 64 + 4], out=buf)
    with pytest.raises(FlasheError):
        eng.philox_random_dev([g], [4], out=buf, offsets=[2 ** 64 + 8])
    with pytest.raises(FlasheError):
        eng.philox_random_dev([g], [-1], out=buf)
    eng.sync()
    assert buf.download(np.float64, 64).tobytes() == np.full(64, CANARY).tobytes()
    assert _unmoved(g, before)


def test_state_dicts_are_advanced_in_place(eng):
    for pre in (0, 3):
        g, ref = _gen(KEYS[1], COUNTERS["carry"], pre), _gen(KEYS[1], COUNTERS["carry"], pre)
        st, before = g.bit_generator.state, g.bit_generator.state
        out = eng.philox_random_dev([st], [4097])
        assert out.download(np.float64, 4097).tobytes() == ref.random(4097).tobytes()
        want = ref.bit_generator.state
        assert st["buffer_pos"] == want["buffer_pos"] and np.array_equal(st["state"]["counter"], want["state"]["counter"])
        assert np.array_equal(st["buffer"], want["buffer"]) and (st["has_uint32"], st["uinteger"]) == (want["has_uint32"], want["uinteger"])
        assert _unmoved(g, before)                                                        # the dict moved, the generator it came from did not


def test_the_call_is_refused_in_a_capture():
    """On an engine of its own between graph_begin and graph_end: refused, nothing written or advanced, and the capture still ends."""
    from flashe_amd import Engine
    from flashe_amd._lib import FlasheError
    e2 = Engine(KEY, 64)
    g = _gen(KEYS[0], COUNTERS["zero"], 1)
    before = g.bit_generator.state
    buf = e2.upload(np.full(16, CANARY))
    e2.sync()
    e2.graph_begin()
    try:
        with pytest.raises(FlasheError):
            e2.philox_random_dev([g], [4], out=buf)
    finally:
        try:
            e2.graph_end()
        except Exception:
            pass
    e2.sync()
    assert _unmoved(g, before) and buf.download(np.float64, 16).tobytes() == np.full(16, CANARY).tobytes()
