"""GPU, ABI level: a precompute cohort's online launch that generates its PCG64 / PCG64DXSM draws itself
(flashe_quantize_combine_cohort_pcg64_dev / _u32_dev) against NumPy's own generator plus the existing launch: a copy of the generator(s)
draws on the host, the numbers are uploaded, flashe_quantize_combine_cohort_dev runs with the same hand-made masks, and the new call must
give the same ciphertexts and sum and leave its generators where the copies stand -- the whole state dict, and the next five draws.  Layer
tables of test_gpu_cohort_prepared (arbitrary alignments, a partial last run of four), float32 and float64 rows in one model, every
element type, every stream position, a cached 32-bit word, states and increments set by hand, the stride path on the chip's real grid,
and the refusals.  Everything is compared as integer arrays; outputs are poisoned with 0xA5 first."""
import copy

import numpy as np
import pytest

from test_gpu_cohort import KEY
from test_gpu_cohort_prepared import HEADS, N, _Cohort, _alloc, _elem_bytes, _get, _same, _sizes
from test_gpu_cohort_prepared_philox import WIDTHS, _host_draws, _masks, _refused, _table

pytestmark = pytest.mark.gpu

M128 = 2 ** 128 - 1
NAMES = ["PCG64", "PCG64DXSM"]


@pytest.fixture(scope="module")
def E():
    from flashe_amd import engine
    return engine


def _pcg(seed, pre=0, name="PCG64", hand=None, cached=False):
    """A Generator over PCG64 or PCG64DXSM: hand = (state, inc) set by hand (None keeps one); cached: one 32-bit draw first, which leaves
    has_uint32 = 1 and the other half of its word in uinteger; then pre values drawn."""
    g = np.random.Generator(getattr(np.random, name)(seed))
    if hand is not None:
        st = g.bit_generator.state
        for k, v in zip(("state", "inc"), hand):
            if v is not None:
                st["state"][k] = v
        g.bit_generator.state = st
    if cached:
        g.integers(0, 2 ** 32, dtype=np.uint32)
        assert g.bit_generator.state["has_uint32"] == 1
    if pre:
        g.random(pre)
    return g


def _check(E, eng, co, rng, compact, with_sum=True, what=()):
    """the new call from rng against the existing launch on the draws of a copy of rng; then the states and the next draws"""
    C, n = co.C, co.n
    ref = copy.deepcopy(rng)                                          # (a list that names one Generator twice keeps doing so)
    masks = _masks(eng, n, C, compact, 17 * C + n)
    du = eng.upload(_host_draws(ref, C, n))
    want_ct, want_sum = [_alloc(eng, n, compact) for _ in range(C)], _alloc(eng, n, compact)
    assert eng.quantize_combine_cohort_dev(n, co.rows, co.srcs, co.dts, co.bits, du, masks, want_ct, want_sum if with_sum else None, compact=compact) is True
    cts, dsum = [_alloc(eng, n, compact) for _ in range(C)], _alloc(eng, n, compact)
    gens, counts, offsets = _table(rng, C, n)
    assert eng.quantize_combine_cohort_pcg64_dev(n, co.rows, co.srcs, co.dts, co.bits, gens, counts, offsets, masks, cts, dsum if with_sum else None,
                                                 compact=compact) is True
    for c in range(C):
        _same(_get(eng, cts[c], n, compact), _get(eng, want_ct[c], n, compact), *what, "client", c)
    _same(_get(eng, dsum, n, compact), _get(eng, want_sum, n, compact), *what, "sum")
    if not with_sum:
        poison = 0xA5A5A5A5 if compact else 0xA5A5A5A5A5A5A5A5
        assert (_get(eng, dsum, n, compact) == np.uint64(poison)).all()
    pairs = list(zip(*(rng, ref) if isinstance(rng, list) else ([rng], [ref])))
    for g, r in pairs:
        assert g.bit_generator.state == r.bit_generator.state, (what, g.bit_generator.state, r.bit_generator.state)
    for g, r in pairs:
        assert np.array_equal(g.random(5), r.random(5)), what


@pytest.mark.parametrize("head", HEADS, ids=["issue-sizes", "no-start-on-4"])
@pytest.mark.parametrize("b,bits,compact", WIDTHS)
def test_the_inline_draws_are_numpys_at_every_width_and_group(E, b, bits, compact, head):
    """Two limbs, one limb and compact (27 has no compiled width); C = 1, 2, 3, 10: whole groups of kPrepCohortGroup and a remainder.  One
    shared generator that has drawn C values: with N % 4 = 1 the clients' stretches start at every residue mod 4.  PCG64DXSM at C = 3."""
    eng = E.Engine(KEY, b, device=0)
    assert N % 4 == 1
    for C in (1, 2, 3, 10):
        co = _Cohort(E, eng, bits, 16, C, _sizes(head), refs=False)
        _check(E, eng, co, _pcg(100 + C, pre=C), compact, what=(b, compact, C))
        if C == 3:
            _check(E, eng, co, _pcg(200 + C, pre=C, name="PCG64DXSM"), compact, what=(b, compact, C, "dxsm"))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("b,bits,compact", [(128, 16, False), (64, 16, False), (20, 16, True)])
def test_every_generator_state(E, b, bits, compact, name):
    """One shared generator that has drawn 0 .. 4 values; one with a cached 32-bit word (has_uint32 = 1: it must survive); an inc set by hand
    to an even value and to 0; a state of 2^128 - 1; a list of per-client generators pre-drawn by different counts; the same Generator
    three times in a list; a null sum.  Five clients each."""
    eng = E.Engine(KEY, b, device=0)
    co = _Cohort(E, eng, bits, 16, 5, _sizes(HEADS[1]), refs=False)
    for pre in range(5):
        _check(E, eng, co, _pcg(7, pre=pre, name=name), compact, what=(b, name, "pre", pre))
    g = _pcg(8, pre=2, name=name, cached=True)
    cached = g.bit_generator.state["uinteger"]
    _check(E, eng, co, g, compact, what=(b, name, "has_uint32"))
    assert g.bit_generator.state["has_uint32"] == 1 and g.bit_generator.state["uinteger"] == cached
    _check(E, eng, co, _pcg(9, pre=1, name=name, hand=(None, 0x9E3779B97F4A7C15F39CC0605CEDC834)), compact, what=(b, name, "even inc"))
    _check(E, eng, co, _pcg(9, name=name, hand=(12345, 0)), compact, what=(b, name, "inc 0"))
    _check(E, eng, co, _pcg(10, name=name, hand=(M128, None)), compact, what=(b, name, "state 2^128 - 1"))
    _check(E, eng, co, _pcg(10, pre=3, name=name, hand=(M128, M128)), compact, what=(b, name, "state and inc 2^128 - 1"))
    _check(E, eng, co, [_pcg(20 + c, pre=3 * c + (c == 4), name=name) for c in range(5)], compact, what=(b, name, "list"))
    a, z = _pcg(31, pre=2, name=name), _pcg(32, name=name)
    _check(E, eng, co, [a, z, a, _pcg(33, pre=1, name=name), a], compact, what=(b, name, "one generator three times"))
    _check(E, eng, co, _pcg(9, pre=3, name=name), compact, with_sum=False, what=(b, name, "null sum"))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("b,bits,compact", [(128, 16, False), (20, 16, True)])
def test_the_stride_path_on_the_chips_grid(E, b, bits, compact, name):
    """n = 2 (1024 W) + 1024 x 3 + 7 values for the W workgroups of the full chip: two whole passes, a partial one and a 3-value tail -- below
    one pass the lane's jump is never composed with the stride jump, so this is the smallest shape at which that code runs.  C = 2, both
    reading client 0's model, from one shared generator at an odd position."""
    eng = E.Engine(KEY, b, device=0)
    W = eng.pcg64_cohort_grid(2 ** 40)
    n = 2 * (1024 * W) + 1024 * 3 + 7
    assert eng.pcg64_cohort_grid(n) == W and W >= 1
    co = _Cohort(E, eng, bits, 16, 2, _sizes(HEADS[1], n), alias=True, refs=False)
    _check(E, eng, co, _pcg(51, pre=3, name=name), compact, what=(b, name, W, n))


@pytest.mark.parametrize("b,bits,compact", [(128, 16, False), (20, 16, True)])
def test_a_plan_table_of_128_clients(E, b, bits, compact):
    """C = 128 at n = 1003, all reading client 0's model: a shared generator, and 128 generators of their own (PCG64DXSM)."""
    eng = E.Engine(KEY, b, device=0)
    co = _Cohort(E, eng, bits, 16, 128, _sizes([1, 6, 0, 301, 256 + 91], 1003), alias=True, refs=False)
    _check(E, eng, co, _pcg(61, pre=1), compact, what=(b, "shared"))
    _check(E, eng, co, [_pcg(1000 + c, pre=c % 7, name="PCG64DXSM") for c in range(128)], compact, what=(b, "list"))


@pytest.mark.parametrize("b,bits,compact", [(128, 16, False), (20, 16, True)])
def test_a_model_of_three_values(E, b, bits, compact):
    """n = 3: no whole run of four, the value-by-value path alone (two layers: the run crosses a boundary too)."""
    eng = E.Engine(KEY, b, device=0)
    co = _Cohort(E, eng, bits, 16, 3, [1, 2], refs=False)
    for name in NAMES:
        _check(E, eng, co, _pcg(71, pre=1, name=name), compact, what=(b, name, "n = 3"))
        _check(E, eng, co, [_pcg(72 + c, pre=c, name=name) for c in range(3)], compact, what=(b, name, "n = 3, list"))


@pytest.mark.parametrize("b,compact", [(128, False), (64, False), (20, True)])
def test_refusals_leave_the_outputs_and_the_generators_alone(E, b, compact):
    from flashe_amd import _lib
    eng = E.Engine(KEY, b, device=0)
    n, C, eb = 1001, 2, _elem_bytes(eng, compact)
    x = [eng.upload(np.zeros(n, np.float32)) for _ in range(C)]
    masks = [_alloc(eng, n + 4, compact, fill=0) for _ in range(C)]
    cts = [_alloc(eng, n + 4, compact) for _ in range(C)]
    dsum = _alloc(eng, n + 4, compact)
    rows = [(0, None, 1.0, 0.0, _lib.TENSOR_F32, 0)]
    srcs, dts = [[d.ptr] for d in x], [[_lib.TENSOR_F32]] * C
    g = [_pcg(71, pre=1), _pcg(72, pre=2)]
    before = copy.deepcopy(g)

    def call(gens=g, counts=(n, n), offsets=(0, n), n=n, srcs=srcs, dts=dts, masks=masks, cts=cts, dsum=dsum):
        return lambda: eng.quantize_combine_cohort_pcg64_dev(n, rows, srcs, dts, 16, list(gens), list(counts), list(offsets), masks, cts, dsum, compact=compact)

    def neither():
        """a variant that is neither: the table the binding builds, one variant word overwritten, through the library's own entry point"""
        arr, nl = eng._tensor_layers(rows)
        _C, ps, pd = eng._cohort_sources(srcs, dts, nl)
        pm, _a = eng._ptr_array(masks)
        pc, _b = eng._ptr_array(cts)
        segs, counts, _o, _hand_back = E._draw_table(E._Pcg64Draws, g, [n, n], [0, n])
        segs[1].variant = 2
        fn = eng._lib.flashe_quantize_combine_cohort_pcg64_u32_dev if compact else eng._lib.flashe_quantize_combine_cohort_pcg64_dev
        return eng._took(fn(eng._h, C, n, arr, nl, ps, pd, 16, segs, len(counts), pm, pc, eng._ptr(dsum)))

    assert "variant" in _refused(E, neither)
    assert "tile" in _refused(E, call(offsets=(0, n + 1)))                       # a gap (and an overrun)
    assert "tile" in _refused(E, call(counts=(n - 1, n)))                        # a gap inside
    assert "overlap" in _refused(E, call(offsets=(0, n - 1)))
    assert "tile" in _refused(E, call(counts=(n, n + 1)))                        # beyond C n
    assert "tile" in _refused(E, call(gens=[g[0]], counts=[2 * n - 1], offsets=[0]))
    assert "tile" in _refused(E, call(gens=[g[0]], counts=[2 * n + 1], offsets=[0]))
    assert "one segment" in _refused(E, call(counts=(n + 1, n - 1), offsets=(0, n + 1)))
    assert "one variant" in _refused(E, call(gens=[g[0], _pcg(73, name="PCG64DXSM")]))     # a table that mixes PCG64 and PCG64DXSM
    _refused(E, lambda: eng.quantize_combine_cohort_pcg64_dev(n, rows, [], [], 16, [g[0]], [0], [0], [], [], dsum, compact=compact))     # n_clients 0
    half = eb // 2
    assert "aligned" in _refused(E, call(cts=[cts[0], cts[1].ptr + half]))
    assert "alias" in _refused(E, call(dsum=masks[1]))
    poison = 0xA5A5A5A5 if compact else 0xA5A5A5A5A5A5A5A5
    assert all((_get(eng, d, n, compact) == np.uint64(poison)).all() for d in cts + [dsum])
    assert all(a.bit_generator.state == z.bit_generator.state for a, z in zip(g, before))
    # an empty model: FLASHE_OK, nothing written, nothing advanced
    none, codes = [[None]] * 2, [[_lib.TENSOR_F32]] * 2
    assert eng.quantize_combine_cohort_pcg64_dev(0, rows, none, codes, 16, g, [0, 0], [0, 0], masks, cts, dsum, compact=compact) is True
    assert eng.quantize_combine_cohort_pcg64_dev(0, rows, none, codes, 16, [g[0]], [0], [0], masks, cts, None, compact=compact) is True
    assert all((_get(eng, d, n, compact) == np.uint64(poison)).all() for d in cts + [dsum])
    assert all(a.bit_generator.state == z.bit_generator.state for a, z in zip(g, before))
    # and the call they were derived from is taken and advances both
    assert call()() is True
    for a, z in zip(g, before):
        z.random(n)
        assert a.bit_generator.state == z.bit_generator.state


def test_the_compact_form_needs_a_compact_ctx(E):
    """_u32 at int_bits 64: FLASHE_EINVAL, the generator untouched."""
    from flashe_amd import _lib
    eng = E.Engine(KEY, 64, device=0)
    n = 100
    x = eng.upload(np.zeros(n, np.float32))
    m, ct = _alloc(eng, n, True, fill=0), _alloc(eng, n, True)
    g = _pcg(81)
    before = copy.deepcopy(g)
    _refused(E, lambda: eng.quantize_combine_cohort_pcg64_dev(n, [(0, None, 1.0, 0.0, _lib.TENSOR_F32, 0)], [[x.ptr]], [[_lib.TENSOR_F32]], 16, [g], [n], [0],
                                                              [m], [ct], None, compact=True))
    assert g.bit_generator.state == before.bit_generator.state
    assert (_get(eng, ct, n, True) == np.uint64(0xA5A5A5A5)).all()
