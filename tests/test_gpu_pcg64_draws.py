"""GPU: Engine.pcg64_random_dev (flashe_pcg64_random_dev: pcg64_random_args_kernel / pcg64_random_table_kernel, either variant) against
Generator(np.random.PCG64(...)).random(n) and Generator(np.random.PCG64DXSM(...)).random(n), compared as bytes: the lengths around one
draw, one wave, a lane's stretch, the workgroup's stride and one tile, the lengths either side of a workgroup's second trip through its
loop (read from the launcher's grid rule on a ctx limited to one CU), generators taken after 0 .. 3 host draws and after a 32-bit draw
that leaves a cached word, states and increments set by hand to 0, 2^128 - 1 and an even value, an output pointer 8 bytes past a 16- and
a 32-byte boundary, several ragged and empty segments of both variants in one call, 128 segments and the counts either side of where the
table leaves the kernel arguments, the same generator twice -- with canary values either side of every range that must come back intact,
and the host generator continuing NumPy's own stream afterwards, a 32-bit draw included -- and the refusals, which advance and write
nothing."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M128 = 2 ** 128 - 1
KEY = bytes(range(32))
CANARY = -7.25
VARIANTS = ["PCG64", "PCG64DXSM"]
HAND = {"state-zero": (0, 0x5851F42D4C957F2D14057B7EF767814F), "state-ones": (M128, 0x5851F42D4C957F2D14057B7EF767814F), "inc-ones": (0x0123456789ABCDEFFEDCBA9876543210, M128),
        "inc-even": (0x0123456789ABCDEFFEDCBA9876543210, 2 ** 65 + 6), "inc-zero": (12345, 0)}


def _gen(name, seed, pre=0, hand=None):
    """A generator of the variant: seeded, `pre` host draws taken (pre = "u32": a 32-bit draw instead, which leaves has_uint32 = 1), or with
    (state, inc) set by hand."""
    g = np.random.Generator(getattr(np.random, name)(seed))
    if hand is not None:
        st = g.bit_generator.state
        st["state"]["state"], st["state"]["inc"] = hand
        g.bit_generator.state = st
    if pre == "u32":
        g.integers(0, 2 ** 32, dtype=np.uint32)
        assert g.bit_generator.state["has_uint32"] == 1
    else:
        g.random(pre)
    return g


@pytest.fixture(scope="module")
def eng():
    from flashe_amd import Engine
    e = Engine(KEY, 64)
    e.set_cu_limit(1)                               # 8 workgroups: a second trip from 8 tiles (32,768 draws) on
    return e


def _check(eng, specs, lead=4, gap=3, shift=0, repeat=None):
    """specs: (variant, seed, pre, hand, n) per segment, laid out `gap` draws apart from draw `lead` of a canary-filled buffer whose address
    the call is given `shift` draws in.  Every range against NumPy, everything else untouched, and the generators continue NumPy's stream."""
    gens = [_gen(v, s, pre, hand) for v, s, pre, hand, _n in specs]
    refs = [_gen(v, s, pre, hand) for v, s, pre, hand, _n in specs]
    counts = [n for *_x, n in specs]
    if repeat is not None:                          # segment `repeat` draws from segment 0's generator, continuing it
        gens[repeat] = gens[0]
    offsets, at = [], lead
    for n in counts:
        offsets.append(at)
        at += n + gap
    total = shift + at + 5
    buf = eng.upload(np.full(total, CANARY))
    out = eng.pcg64_random_dev(gens, counts, out=buf.ptr + 8 * shift, offsets=offsets)
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
        assert g.bit_generator.state == r.bit_generator.state, s                 # state, inc, has_uint32, uinteger
        assert g.integers(0, 2 ** 32, 3, dtype=np.uint32).tobytes() == r.integers(0, 2 ** 32, 3, dtype=np.uint32).tobytes(), s
        assert g.random(7).tobytes() == r.random(7).tobytes(), s
        assert g.bit_generator.state == r.bit_generator.state, s


def test_the_grid_rule(eng):
    cap, tiles, tile = eng.pcg64_grid(1 << 30)
    assert cap == 8 and tile == 256 * eng.PCG64_STRETCH and tiles == (1 << 30) // tile          # (one CU: stream_grid's 8 workgroups per CU)
    assert eng.pcg64_grid(tile)[:2] == (1, 1) and eng.pcg64_grid(tile + 1)[:2] == (2, 2) and eng.pcg64_grid(0)[1] == 0


# 1, 2; a wave (64); a lane's stretch R = 16; the workgroup's stride (256: where a lane's second draw starts); a tile (256 R = 4,096)
@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097])
@pytest.mark.parametrize("variant", VARIANTS)
def test_lengths_around_a_wave_a_stretch_and_a_tile(eng, variant, n):
    assert eng.PCG64_STRETCH == 16 and eng.pcg64_grid(1)[2] == 4096
    _check(eng, [(variant, 3, 1, None, n)], lead=4)                                      # a 32-byte aligned range
    _check(eng, [(variant, 3, 2, None, n)], lead=1)                                      # 8 bytes past a 32-byte boundary
    _check(eng, [(variant, 3, 0, None, n)], lead=3)                                      # 8 bytes past a 16-byte boundary only
    _check(eng, [(variant, 3, 3, None, n)], lead=2, shift=1)


@pytest.mark.parametrize("variant", VARIANTS)
def test_lengths_either_side_of_a_workgroups_second_trip(eng, variant):
    cap, _tiles, tile = eng.pcg64_grid(1 << 30)
    n2 = cap * tile + 1                                                                  # the first length that needs tile cap + 1
    assert eng.pcg64_grid(n2 - 1)[:2] == (cap, cap) and eng.pcg64_grid(n2)[:2] == (cap, cap + 1)
    for n in (n2 - 1, n2, n2 + 1):
        _check(eng, [(variant, 11, 1, None, n)], lead=3)


@pytest.mark.parametrize("pre", [0, 1, 2, 3, "u32"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_generators_taken_after_host_draws_and_with_a_cached_word(eng, variant, pre):
    _check(eng, [(variant, 5, pre, None, 4099)], lead=5)
    _check(eng, [(variant, 5, pre, None, 3)], lead=1)


@pytest.mark.parametrize("hand", list(HAND))
@pytest.mark.parametrize("variant", VARIANTS)
def test_states_and_increments_set_by_hand(eng, variant, hand):
    for pre in (0, "u32"):
        _check(eng, [(variant, 1, pre, HAND[hand], 2 * 4096 + 259)], lead=1)


def test_several_ragged_and_empty_segments_of_both_variants_in_one_call(eng):
    a, b = VARIANTS
    specs = [(a, 1, 0, None, 5), (b, 2, 2, None, 4099), (a, 3, "u32", HAND["inc-even"], 1), (b, 4, 1, HAND["state-ones"], 8193)]
    _check(eng, specs, lead=1, gap=0)                                                    # back to back
    _check(eng, specs, lead=2, gap=1)
    _check(eng, [(a, 1, 1, None, 4097), (a, 2, 0, None, 4097)], lead=0, gap=0)           # the K + 1 shape
    _check(eng, [(b, 1, 1, None, 4097), (b, 2, 0, None, 4097)], lead=3, gap=0, shift=1)
    _check(eng, [(a, 1, 0, None, 0), (b, 1, 2, None, 9), (a, 1, 3, None, 0), (a, 1, 3, None, 300), (b, 9, 0, None, 0)])      # empty segments
    _check(eng, [(a, 1, 0, None, 0), (b, 1, 2, None, 0)])                               # nothing at all


def test_128_segments_and_either_side_of_the_kernel_argument_table(eng):
    one = [(VARIANTS[0], s, s % 4, None, 1 + (37 * s) % 1500) for s in range(128)]
    _check(eng, one, lead=1, gap=1)                                                      # 128 plans of one variant: the ctx table
    _check(eng, one[:49], lead=2, gap=0)                                                 # the first count the table kernel takes
    _check(eng, one[:48], lead=2, gap=0)                                                 # the last the kernel arguments hold
    dx = [(VARIANTS[1], s, "u32" if s % 5 == 0 else s % 4, None, 1 + (41 * s) % 1700) for s in range(49)]
    _check(eng, dx, lead=3, gap=2)
    _check(eng, dx[:48], lead=3, gap=2)
    # both variants in one call: each has a table of its own -- in the arguments up to 48 segments, else side by side in the ctx buffer
    mixed = [(VARIANTS[s % 2], s, s % 4, None, 1 + (53 * s) % 1300) for s in range(128)]
    _check(eng, mixed, lead=0, gap=0)                                                    # 64 + 64: both in the ctx buffer
    _check(eng, mixed[:98], lead=0, gap=0)                                               # 49 + 49
    _check(eng, mixed[:97], lead=0, gap=0)                                               # 49 in the ctx buffer, 48 in the arguments
    uneven = [(VARIANTS[1 if s % 3 == 0 else 0], s, s % 4, None, (53 * s) % 1300) for s in range(128)]     # 85 + 43, two of them empty
    _check(eng, uneven, lead=1, gap=1)


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_same_generator_twice_continues_itself(eng, variant):
    other = VARIANTS[1 - VARIANTS.index(variant)]
    _check(eng, [(variant, 8, 1, None, 1030), (other, 3, 0, None, 17), (variant, 8, 1, None, 4100)], repeat=2)
    _check(eng, [(variant, 8, "u32", None, 0), (variant, 8, "u32", None, 70)], repeat=1)


def test_state_dicts_are_advanced_in_place(eng):
    for variant in VARIANTS:
        g, ref = _gen(variant, 6, "u32"), _gen(variant, 6, "u32")
        st = g.bit_generator.state
        out = eng.pcg64_random_dev([st], [4097])
        assert out.download(np.float64, 4097).tobytes() == ref.random(4097).tobytes()
        assert st == ref.bit_generator.state and g.bit_generator.state != st              # the dict moved, the generator it came from did not


def _refused_in_a_capture(variant):
    """The call on an engine of its own between graph_begin and graph_end: refused, and the capture still ends."""
    from flashe_amd import Engine
    from flashe_amd._lib import FlasheError
    e2 = Engine(KEY, 64)
    g = _gen(variant, 1)
    before = g.bit_generator.state
    buf = e2.upload(np.full(16, CANARY))
    e2.sync()
    e2.graph_begin()
    try:
        with pytest.raises(FlasheError):
            e2.pcg64_random_dev([g], [4], out=buf)
    finally:
        try:
            e2.graph_end()
        except Exception:
            pass
    e2.sync()
    return g.bit_generator.state == before and buf.download(np.float64, 16).tobytes() == np.full(16, CANARY).tobytes()


def test_the_refusals_advance_and_write_nothing(eng):
    from flashe_amd._lib import FlasheError
    g, h = _gen("PCG64", 1, 2), _gen("PCG64DXSM", 2, "u32")
    buf = eng.upload(np.full(64, CANARY))
    before = (g.bit_generator.state, h.bit_generator.state)
    with pytest.raises(FlasheError):
        eng.pcg64_random_dev([g, h], [10, 10], out=buf, offsets=[0, 9])                      # overlapping ranges
    with pytest.raises(FlasheError):
        eng.pcg64_random_dev([g], [2 ** 60 + 1], out=buf)                                    # overflow: n
    with pytest.raises(FlasheError):
        eng.pcg64_random_dev([g, h], [4, 4], out=buf, offsets=[0, 2 ** 60 - 3])              # overflow: offset + n
    with pytest.raises(FlasheError):
        eng.pcg64_random_dev([g], [2 ** 64 + 4], out=buf)                                    # a count that does not fit the table's word
    with pytest.raises(FlasheError):
        eng.pcg64_random_dev([g, h], [4, 4], out=buf.ptr + 4)                                # a misaligned output
    for other in (np.random.Philox(1), np.random.SFC64(1), np.random.MT19937(1)):
        with pytest.raises(FlasheError):
            eng.pcg64_random_dev([g, np.random.Generator(other)], [4, 4], out=buf)           # another bit generator
    with pytest.raises(ValueError):
        eng.pcg64_random_dev([g] * 129, [0] * 129, out=buf)
    with pytest.raises(ValueError):
        eng.pcg64_random_dev([g, h], [4], out=buf)
    bad = g.bit_generator.state
    bad["state"]["state"] = 2 ** 128
    with pytest.raises(FlasheError):
        eng.pcg64_random_dev([h, bad], [4, 4], out=buf)
    # the C entry point itself: a variant above 1
    from flashe_amd import _lib
    seg = (_lib.Pcg64Segment * 1)()
    seg[0].variant, seg[0].n = 2, 4
    assert eng._lib.flashe_pcg64_random_dev(eng._h, seg, 1, buf.ptr) == -22 and list(seg[0].state) == [0, 0]
    eng.sync()
    assert buf.download(np.float64, 64).tobytes() == np.full(64, CANARY).tobytes()
    assert (g.bit_generator.state, h.bit_generator.state) == before
    for variant in VARIANTS:
        assert _refused_in_a_capture(variant)
