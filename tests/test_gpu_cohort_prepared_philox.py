"""GPU, ABI level: a precompute cohort's online launch that generates its Philox draws itself (flashe_quantize_combine_cohort_philox_dev /
_u32_dev) against NumPy's own generator plus the existing launch: a copy of the generator(s) draws on the host, the numbers are
uploaded, flashe_quantize_combine_cohort_dev runs with the same hand-made masks, and the new call must give the same ciphertexts and sum
and leave its generators where the copies stand.  Layer tables of test_gpu_cohort_prepared (arbitrary alignments, a partial last run of
four), float32 and float64 rows in one model, every element type, every stream position, the counter's carry and wrap inside the
launch, and the refusals.  Everything is compared as integer arrays; outputs are poisoned with 0xA5 first."""
import copy

import numpy as np
import pytest

from test_gpu_cohort import KEY
from test_gpu_cohort_prepared import HEADS, N, _Cohort, _alloc, _elem_bytes, _get, _same, _sizes

pytestmark = pytest.mark.gpu

WIDTHS = [(128, 16, False), (120, 16, False), (64, 16, False), (33, 16, False), (20, 16, True), (27, 16, True)]
M64 = 2 ** 64 - 1


@pytest.fixture(scope="module")
def E():
    from flashe_amd import engine
    return engine


def _philox(seed, pre=0, counter=None, buffer_pos=None):
    """A Generator over Philox: pre values drawn already; counter: the state's counter words set by hand (the buffer then belongs to no
    block: buffer_pos stays 4); buffer_pos: set by hand on a state whose buffer is block(counter) -- after pre = 4 k draws."""
    g = np.random.Generator(np.random.Philox(seed))
    if counter is not None:
        st = g.bit_generator.state
        st["state"]["counter"] = np.array(counter, dtype=np.uint64)
        g.bit_generator.state = st
    if pre:
        g.random(pre)
    if buffer_pos is not None:
        st = g.bit_generator.state
        assert st["buffer_pos"] == 4 and pre and pre % 4 == 0
        st["buffer_pos"] = buffer_pos
        g.bit_generator.state = st
    return g


def _state_equal(a, b):
    sa, sb = a.bit_generator.state, b.bit_generator.state
    return (sa["bit_generator"] == sb["bit_generator"] == "Philox" and sa["buffer_pos"] == sb["buffer_pos"]
            and all(np.array_equal(sa["state"][k], sb["state"][k]) for k in ("counter", "key")) and np.array_equal(sa["buffer"], sb["buffer"])
            and sa["has_uint32"] == sb["has_uint32"] and sa["uinteger"] == sb["uinteger"])


def _masks(eng, n, C, compact, seed):
    """hand-made masks: random words of the element type, not reduced mod 2^b"""
    r = np.random.Generator(np.random.PCG64(seed))
    if compact:
        return [eng.upload(r.integers(0, 2 ** 32, size=max(n, 4), dtype=np.uint64).astype(np.uint32)) for _ in range(C)]
    return [eng.upload(r.integers(0, 2 ** 64, size=max(n * eng.limbs, 2), dtype=np.uint64)) for _ in range(C)]


def _table(rng, C, n):
    """the call's table for rng= as FlasheCohort takes it: one generator for all clients, or a list of one per client"""
    if isinstance(rng, list):
        return rng, [n] * C, [c * n for c in range(C)]
    return [rng], [C * n], [0]


def _host_draws(ref, C, n):
    """what the copies draw on the host, client-major (a generator listed twice continues itself in list order)"""
    if isinstance(ref, list):
        return np.concatenate([g.random(n) for g in ref]) if n else np.zeros(0)
    return ref.random(C * n)


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
    assert eng.quantize_combine_cohort_philox_dev(n, co.rows, co.srcs, co.dts, co.bits, gens, counts, offsets, masks, cts, dsum if with_sum else None,
                                                  compact=compact) is True
    for c in range(C):
        _same(_get(eng, cts[c], n, compact), _get(eng, want_ct[c], n, compact), *what, "client", c)
    _same(_get(eng, dsum, n, compact), _get(eng, want_sum, n, compact), *what, "sum")
    if not with_sum:
        poison = 0xA5A5A5A5 if compact else 0xA5A5A5A5A5A5A5A5
        assert (_get(eng, dsum, n, compact) == np.uint64(poison)).all()
    for g, r in zip(*(rng, ref) if isinstance(rng, list) else ([rng], [ref])):
        assert _state_equal(g, r), (what, g.bit_generator.state, r.bit_generator.state)
    for g, r in zip(*(rng, ref) if isinstance(rng, list) else ([rng], [ref])):
        assert np.array_equal(g.random(5), r.random(5)), what


@pytest.mark.parametrize("head", HEADS, ids=["issue-sizes", "no-start-on-4"])
@pytest.mark.parametrize("b,bits,compact", WIDTHS)
def test_the_inline_draws_are_numpys_at_every_width_and_group(E, b, bits, compact, head):
    """Two limbs, one limb and compact (27 has no compiled width); C = 1, 2, 3, 10: whole groups of kPrepCohortGroup and a remainder.  One
    shared generator that has drawn C values: with N % 4 = 1 the clients cycle through the residues."""
    eng = E.Engine(KEY, b, device=0)
    assert N % 4 == 1
    for C in (1, 2, 3, 10):
        co = _Cohort(E, eng, bits, 16, C, _sizes(head), refs=False)
        _check(E, eng, co, _philox(100 + C, pre=C), compact, what=(b, compact, C))


@pytest.mark.parametrize("b,bits,compact", [(128, 16, False), (64, 16, False), (20, 16, True)])
def test_every_stream_position(E, b, bits, compact):
    """One shared generator at every buffer_pos 0 .. 4 (a fresh one, 1 .. 4 values drawn, and position 0 set by hand on a full buffer), five
    clients each; a list of per-client generators pre-drawn by different counts; the same Generator twice in a list; a null sum."""
    eng = E.Engine(KEY, b, device=0)
    co = _Cohort(E, eng, bits, 16, 5, _sizes(HEADS[1]), refs=False)
    for pre in range(5):
        g = _philox(7, pre=pre)
        assert g.bit_generator.state["buffer_pos"] == (pre or 4)
        _check(E, eng, co, g, compact, what=(b, "pre", pre))
    g = _philox(8, pre=8, buffer_pos=0)
    _check(E, eng, co, g, compact, what=(b, "buffer_pos 0"))
    _check(E, eng, co, [_philox(20 + c, pre=3 * c + (c == 4)) for c in range(5)], compact, what=(b, "list"))
    a, z = _philox(31, pre=2), _philox(32)
    _check(E, eng, co, [a, z, a, _philox(33, pre=1), a], compact, what=(b, "one generator three times"))
    _check(E, eng, co, _philox(9, pre=3), compact, with_sum=False, what=(b, "null sum"))


@pytest.mark.parametrize("b,bits,compact", [(128, 16, False), (20, 16, True)])
def test_the_counter_carries_and_wraps_inside_the_launch(E, b, bits, compact):
    """counter[0] = 2^64 - 3: the carry into word 1 after three blocks; all four words 2^64 - 1: the wrap at 2^256 with the first block.
    Shared (the later clients start beyond the carry) and per client."""
    eng = E.Engine(KEY, b, device=0)
    co = _Cohort(E, eng, bits, 16, 3, _sizes(HEADS[0]), refs=False)
    for counter in ([M64 - 2, 0, 0, 0], [M64 - 2, M64, 5, 0], [M64] * 4, [M64 - 1, M64, M64, M64]):
        for pre in (0, 2):
            _check(E, eng, co, _philox(41, pre=pre, counter=counter), compact, what=(b, counter, pre))
        _check(E, eng, co, [_philox(50 + c, pre=c, counter=counter) for c in range(3)], compact, what=(b, counter, "list"))


@pytest.mark.parametrize("b,bits,compact", [(128, 16, False), (20, 16, True)])
def test_a_plan_table_of_128_clients(E, b, bits, compact):
    """C = 128 at n = 1003, all reading client 0's model: a shared generator, and 128 generators of their own."""
    eng = E.Engine(KEY, b, device=0)
    co = _Cohort(E, eng, bits, 16, 128, _sizes([1, 6, 0, 301, 256 + 91], 1003), alias=True, refs=False)
    _check(E, eng, co, _philox(61, pre=1), compact, what=(b, "shared"))
    _check(E, eng, co, [_philox(1000 + c, pre=c % 7) for c in range(128)], compact, what=(b, "list"))


def _refused(E, call):
    with pytest.raises(E.FlasheError) as ei:
        call()
    assert ei.value.code == -22, ei.value
    return str(ei.value)


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
    g = [_philox(71, pre=1), _philox(72, pre=2)]
    before = copy.deepcopy(g)

    def call(gens=g, counts=(n, n), offsets=(0, n), n=n, srcs=srcs, dts=dts, masks=masks, cts=cts, dsum=dsum):
        return lambda: eng.quantize_combine_cohort_philox_dev(n, rows, srcs, dts, 16, list(gens), list(counts), list(offsets), masks, cts, dsum, compact=compact)

    bad = g[0].bit_generator.state
    bad["buffer_pos"] = 5
    assert "buffer_pos" in _refused(E, call(gens=[bad, g[1]]))
    assert "tile" in _refused(E, call(offsets=(0, n + 1)))                       # a gap (and an overrun)
    assert "tile" in _refused(E, call(counts=(n - 1, n)))                        # a gap inside
    assert "overlap" in _refused(E, call(offsets=(0, n - 1)))
    assert "tile" in _refused(E, call(counts=(n, n + 1)))                        # beyond C n
    assert "tile" in _refused(E, call(gens=[g[0]], counts=[2 * n - 1], offsets=[0]))
    assert "tile" in _refused(E, call(gens=[g[0]], counts=[2 * n + 1], offsets=[0]))
    assert "one segment" in _refused(E, call(counts=(n + 1, n - 1), offsets=(0, n + 1)))
    _refused(E, lambda: eng.quantize_combine_cohort_philox_dev(n, rows, [], [], 16, [g[0]], [0], [0], [], [], dsum, compact=compact))     # n_clients 0
    half = eb // 2
    assert "aligned" in _refused(E, call(cts=[cts[0], cts[1].ptr + half]))
    assert "alias" in _refused(E, call(dsum=masks[1]))
    poison = 0xA5A5A5A5 if compact else 0xA5A5A5A5A5A5A5A5
    assert all((_get(eng, d, n, compact) == np.uint64(poison)).all() for d in cts + [dsum])
    assert all(_state_equal(a, z) for a, z in zip(g, before))
    # an empty model: FLASHE_OK, nothing written, nothing advanced
    none, codes = [[None]] * 2, [[_lib.TENSOR_F32]] * 2
    assert eng.quantize_combine_cohort_philox_dev(0, rows, none, codes, 16, g, [0, 0], [0, 0], masks, cts, dsum, compact=compact) is True
    assert eng.quantize_combine_cohort_philox_dev(0, rows, none, codes, 16, [g[0]], [0], [0], masks, cts, None, compact=compact) is True
    assert all((_get(eng, d, n, compact) == np.uint64(poison)).all() for d in cts + [dsum])
    assert all(_state_equal(a, z) for a, z in zip(g, before))
    # and the call they were derived from is taken and advances both
    assert call()() is True
    for a, z in zip(g, before):
        z.random(n)
        assert _state_equal(a, z)


def test_the_compact_form_needs_a_compact_ctx(E):
    """_u32 at int_bits 64: FLASHE_EINVAL, the generator untouched."""
    from flashe_amd import _lib
    eng = E.Engine(KEY, 64, device=0)
    n = 100
    x = eng.upload(np.zeros(n, np.float32))
    m, ct = _alloc(eng, n, True, fill=0), _alloc(eng, n, True)
    g = _philox(81)
    before = copy.deepcopy(g)
    _refused(E, lambda: eng.quantize_combine_cohort_philox_dev(n, [(0, None, 1.0, 0.0, _lib.TENSOR_F32, 0)], [[x.ptr]], [[_lib.TENSOR_F32]], 16, [g], [n], [0],
                                                               [m], [ct], None, compact=True))
    assert _state_equal(g, before)
    assert (_get(eng, ct, n, True) == np.uint64(0xA5A5A5A5)).all()
