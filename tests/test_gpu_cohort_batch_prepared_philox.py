"""GPU, ABI level: a BATCHED precompute cohort's online launch that generates its Philox draws itself
(flashe_quantize_batch_combine_cohort_philox_dev) against NumPy's own generator plus the existing launch: a deep copy of the generator(s)
draws on the host, the numbers are uploaded, flashe_quantize_batch_combine_cohort_dev runs with the same hand-made masks, and the new
call must give the same ciphertexts and sum and leave its generators where the copies stand, the next five draws equal.  Every case of
test_the_batched_online_launch_is_every_clients_quantise_batch_encrypt (bs 6, 5, 7 compiled in; 3 at one limb, 2 and 1 at run time;
rows that end in fewer than four elements and in pads; float32 and float64 rows in one model), every stream position, the counter's
carry and wrap inside the launch, 128 plans, a null sum, an empty model, and the refusals.  Integers are compared as bytes; outputs
are poisoned with 0xA5 first."""
import copy

import numpy as np
import pytest

from test_gpu_cohort import KEY
from test_gpu_cohort_batch import _elems_to_sizes, _field_bits
from test_gpu_cohort_prepared import _Cohort, _alloc, _get, _same
from test_gpu_cohort_prepared_philox import M64, _host_draws, _masks, _philox, _refused, _state_equal, _table

pytestmark = pytest.mark.gpu

POISON = np.uint64(0xA5A5A5A5A5A5A5A5)


@pytest.fixture(scope="module")
def E():
    from flashe_amd import engine
    return engine


def _n_elems(sizes, bs):
    return sum(-(-s // bs) for s in sizes)


def _small_sizes(bs):
    """A model of a few thousand values with more groups of four elements than one workgroup has lanes: a one-value layer, an empty one,
    a row of whole groups, rows that end in 2, 1 and 3 elements, last elements with 1 and bs - 1 values (bs > 1); n_values % 4 = 1."""
    sizes = [1, 0, 8 * bs, 6 * bs - (bs > 1), 1101 * bs - (bs - 1), 23 * bs]
    sizes.append(5 - sum(sizes) % 4 if sum(sizes) % 4 != 1 else 4)
    assert sum(sizes) % 4 == 1 and _n_elems(sizes, bs) // 4 > 256
    return sizes


class _Job:
    def __init__(self, E, b, num_clients, field_bits, C, sizes, alias=False, bits=16):
        self.eng = eng = E.Engine(KEY, b, device=0)
        self.fb = fb = field_bits or _field_bits(num_clients)
        self.bs, self.bits = b // fb, bits
        self.co = _Cohort(E, eng, bits, 16, C, sizes, refs=False, alias=alias)
        self.C, self.n, self.n_elems = C, self.co.n, _n_elems(sizes, self.bs)

    def call(self, rng, masks, cts, dsum, n=None, n_elems=None, fb=None, table=None, eng=None):
        co = self.co
        gens, counts, offsets = table or _table(rng, self.C, self.n if n is None else n)
        return (eng or self.eng).quantize_combine_cohort_philox_dev(self.n if n is None else n, co.rows, co.srcs, co.dts, self.bits, gens, counts, offsets, masks, cts, dsum,
                                                           batch=(self.n_elems if n_elems is None else n_elems, self.fb if fb is None else fb))

    def check(self, rng, with_sum=True, what=()):
        """the new call from rng against the existing launch on the draws of a deep copy of rng; then the states and the next draws"""
        eng, co, C, n, ne = self.eng, self.co, self.C, self.n, self.n_elems
        ref = copy.deepcopy(rng)                                      # (a list that names one Generator twice keeps doing so)
        masks = _masks(eng, ne, C, False, 17 * C + n)
        du = eng.upload(_host_draws(ref, C, n))
        want_ct, want_sum = [_alloc(eng, ne, False) for _ in range(C)], _alloc(eng, ne, False)
        assert eng.quantize_combine_cohort_dev(n, co.rows, co.srcs, co.dts, self.bits, du, masks, want_ct, want_sum if with_sum else None, batch=(ne, self.fb)) is True
        cts, dsum = [_alloc(eng, ne, False) for _ in range(C)], _alloc(eng, ne, False)
        assert self.call(rng, masks, cts, dsum if with_sum else None) is True
        for c in range(C):
            _same(_get(eng, cts[c], ne, False), _get(eng, want_ct[c], ne, False), *what, "client", c)
        _same(_get(eng, dsum, ne, False), _get(eng, want_sum, ne, False), *what, "sum")
        if not with_sum:
            assert (_get(eng, dsum, ne, False) == POISON).all()
        pairs = list(zip(rng, ref)) if isinstance(rng, list) else [(rng, ref)]
        for g, r in pairs:
            assert _state_equal(g, r), (what, g.bit_generator.state, r.bit_generator.state)
        for g, r in pairs:
            assert np.array_equal(g.random(5), r.random(5)), what


CASES = [(120, 10, None, 10), (120, 10, 24, 3), (128, 2, None, 2), (64, 4, None, 3), (120, 4, 60, 3), (128, 2, 128, 2)]


@pytest.mark.parametrize("b,num_clients,field_bits,C", CASES)
def test_every_case_of_the_batched_online_launch_through_the_inline_call(E, b, num_clients, field_bits, C):
    """The buffer form's cases: one shared generator that has drawn C values (the clients' phases differ), and a list of block-aligned
    generators."""
    fb = field_bits or _field_bits(num_clients)
    bs = b // fb
    assert bs == {(120, None): 6, (120, 24): 5, (128, None): 7, (64, None): 3, (120, 60): 2, (128, 128): 1}[(b, field_bits)]
    sizes = _elems_to_sizes(bs, 6000) if bs > 1 else [1, 0, 100, 27, 640, 5001, 231]
    job = _Job(E, b, num_clients, field_bits, C, sizes)
    assert job.n_elems == 6000
    job.check(_philox(100 + C, pre=C), what=(b, bs, "shared"))
    job.check([_philox(200 + c, pre=4 * c) for c in range(C)], what=(b, bs, "aligned list"))


@pytest.mark.parametrize("field_bits,bs", [(12, 5), (10, 6), (9, 7)])
def test_one_limb_elements_at_the_compiled_sizes(E, field_bits, bs):
    """int_bits 64 with 8-bit values in fields of 12, 10 and 9 bits: the uint64 kernels with five, six and seven values per element."""
    assert 64 // field_bits == bs
    job = _Job(E, 64, 4, field_bits, 3, _small_sizes(bs), bits=8)
    job.check(_philox(90 + bs, pre=3), what=(64, bs, "shared"))
    job.check([_philox(95 + c, pre=4 * c) for c in range(3)], what=(64, bs, "aligned list"))


@pytest.mark.parametrize("b,num_clients,field_bits", [(120, 10, None), (128, 2, None), (120, 10, 24), (64, 4, None)])
def test_every_stream_position(E, b, num_clients, field_bits):
    """One shared generator with 0 .. 4 values drawn and buffer_pos 0 set by hand (n_values % 4 = 1: the clients cycle through the four
    phases); per-client generators pre-drawn by c values; one Generator listed twice; C = 1, 2, 3 and 10."""
    bs = b // (field_bits or _field_bits(num_clients))
    sizes = _small_sizes(bs)
    for C in (1, 2, 3, 10):
        job = _Job(E, b, num_clients, field_bits, C, sizes)
        assert job.n % 4 == 1
        for pre in range(5) if C == 10 else (C,):
            g = _philox(7, pre=pre)
            assert g.bit_generator.state["buffer_pos"] == (pre or 4)
            job.check(g, what=(b, C, "pre", pre))
        job.check(_philox(8, pre=8, buffer_pos=0), what=(b, C, "buffer_pos 0"))
        job.check([_philox(20 + c, pre=c) for c in range(C)], what=(b, C, "list"))
        if C >= 2:
            a = _philox(31, pre=2)
            job.check([a] + [_philox(40 + c, pre=1) for c in range(C - 2)] + [a], what=(b, C, "one generator twice"))


@pytest.mark.parametrize("b,num_clients,field_bits", [(120, 10, None), (128, 2, None), (120, 4, 60)])
def test_the_counter_carries_and_wraps_inside_the_launch(E, b, num_clients, field_bits):
    """counter[0] = 2^64 - 3: the carry into word 1 after three blocks; all four words 2^64 - 1: the wrap at 2^256 with the first block.
    Shared (the later clients start beyond the carry) and per client."""
    bs = b // (field_bits or _field_bits(num_clients))
    job = _Job(E, b, num_clients, field_bits, 3, _small_sizes(bs))
    for counter in ([M64 - 2, 0, 0, 0], [M64 - 2, M64, 5, 0], [M64] * 4, [M64 - 1, M64, M64, M64]):
        for pre in (0, 2):
            job.check(_philox(41, pre=pre, counter=counter), what=(b, counter, pre))
        job.check([_philox(50 + c, pre=c, counter=counter) for c in range(3)], what=(b, counter, "list"))


@pytest.mark.parametrize("b,num_clients,field_bits", [(120, 10, None), (64, 4, None)])
def test_a_plan_table_of_128_clients(E, b, num_clients, field_bits):
    """C = 128 on a small model, all reading client 0's floats: a shared generator, and 128 generators of their own."""
    bs = b // (field_bits or _field_bits(num_clients))
    job = _Job(E, b, num_clients, field_bits, 128, [1, 0, 8 * bs, 6 * bs - 1, 37 * bs + 2], alias=True)
    job.check(_philox(61, pre=1), what=(b, "shared"))
    job.check([_philox(1000 + c, pre=c % 7) for c in range(128)], what=(b, "list"))


@pytest.mark.parametrize("b,num_clients,field_bits", [(120, 10, None), (64, 4, None)])
def test_a_null_sum_and_an_empty_model(E, b, num_clients, field_bits):
    from flashe_amd import _lib
    bs = b // (field_bits or _field_bits(num_clients))
    job = _Job(E, b, num_clients, field_bits, 3, _small_sizes(bs))
    job.check(_philox(9, pre=3), with_sum=False, what=(b, "null sum"))
    eng = job.eng
    d, d2 = _alloc(eng, 4, False), _alloc(eng, 4, False)
    rows = [(0, None, 1.0, 0.0, _lib.TENSOR_F32, 0), (0, None, 1.0, 0.0, _lib.TENSOR_F64, 0)]
    none, codes = [[None, None]] * 2, [[_lib.TENSOR_F32, _lib.TENSOR_F64]] * 2
    g = _philox(10, pre=1)
    before = copy.deepcopy(g)
    for s in (d2, None):
        assert eng.quantize_combine_cohort_philox_dev(0, rows, none, codes, 16, [g], [0], [0], [d, d], [d, d], s, batch=(0, job.fb)) is True
    assert all((_get(eng, v, 4, False) == POISON).all() for v in (d, d2))
    assert _state_equal(g, before)


@pytest.mark.parametrize("b,num_clients,field_bits", [(120, 10, None), (64, 4, None)])
def test_refusals_leave_the_outputs_and_the_generators_alone(E, b, num_clients, field_bits):
    """FLASHE_EINVAL with nothing written and nothing advanced: segments that tile C n_elems and not C n_values, a client split over two
    segments, a gap, buffer_pos 5, 129 segments, an n_elems the layers do not batch into, field_bits above int_bits, a graph being
    captured.  Then the call they were derived from is taken and advances both generators."""
    bs = b // (field_bits or _field_bits(num_clients))
    job = _Job(E, b, num_clients, field_bits, 2, _small_sizes(bs))
    eng, n, ne = job.eng, job.n, job.n_elems
    masks = [_alloc(eng, ne, False, fill=0) for _ in range(2)]
    cts, dsum = [_alloc(eng, ne, False) for _ in range(2)], _alloc(eng, ne, False)
    g = [_philox(71, pre=1), _philox(72, pre=2)]
    before = copy.deepcopy(g)

    def call(gens=g, counts=(n, n), offsets=(0, n), **kw):
        return lambda: job.call(None, masks, cts, dsum, table=(list(gens), list(counts), list(offsets)), **kw)

    assert "tile" in _refused(E, call(counts=(ne, ne), offsets=(0, ne)))                      # the elements, not the values
    assert "tile" in _refused(E, call(gens=[g[0]], counts=[2 * ne], offsets=[0]))
    assert "one segment" in _refused(E, call(counts=(n + 1, n - 1), offsets=(0, n + 1)))      # client 1 spans two segments
    assert "tile" in _refused(E, call(offsets=(0, n + 1)))                                    # a gap
    assert "tile" in _refused(E, call(counts=(n - 1, n)))
    bad = g[0].bit_generator.state
    bad["buffer_pos"] = 5
    assert "buffer_pos" in _refused(E, call(gens=[bad, g[1]]))
    many = [_philox(300 + i) for i in range(129)]
    with pytest.raises(ValueError, match="129 segments"):                                     # (the binding counts them before the library does)
        call(gens=many, counts=[n, n] + [0] * 127, offsets=[0, n] + [0] * 127)()
    # ... and the library's own count, through the entry point itself: a table that is in order but for its 129 segments
    from flashe_amd import _lib
    co = job.co
    arr, nl = eng._tensor_layers(co.rows)
    n_cl, ps, pd = eng._cohort_sources(co.srcs, co.dts, nl)
    (pm, _a), (pc, _b) = eng._ptr_array(masks), eng._ptr_array(cts)
    segs = (_lib.PhiloxSegment * 129)()
    for i in range(129):
        segs[i].key[0], segs[i].buffer_pos, segs[i].n, segs[i].offset = 1 + i, 4, n if i < 2 else 0, n if i == 1 else 0
    raw = lambda count: eng._lib.flashe_quantize_batch_combine_cohort_philox_dev(eng._h, n_cl, n, ne, arr, nl, ps, pd, 16, job.fb, segs, count, pm, pc, eng._ptr(dsum))     # noqa: E731
    with pytest.raises(E.FlasheError) as ei:
        eng._check(raw(129))
    assert ei.value.code == -22 and "129 segments" in str(ei.value)
    assert all(segs[i].buffer_pos == 4 and not any(segs[i].counter) for i in range(129))
    assert "batch into" in _refused(E, call(n_elems=ne + 1))
    assert "batch into" in _refused(E, call(n_elems=ne - 1))
    _refused(E, call(fb=b + 1))
    e2 = E.Engine(KEY, b, device=0)                                   # (an engine of its own between graph_begin and graph_end)
    eng.sync()
    e2.graph_begin()
    try:
        msg = _refused(E, call(eng=e2))
    finally:
        try:
            e2.graph_end()
        except Exception:
            pass
    e2.sync()
    assert "replay" in msg
    assert all((_get(eng, d, ne, False) == POISON).all() for d in cts + [dsum])
    assert all(_state_equal(a, z) for a, z in zip(g, before))
    assert all(_state_equal(a, _philox(300 + i)) for i, a in enumerate(many))
    assert call()() is True
    for a, z in zip(g, before):
        z.random(n)
        assert _state_equal(a, z)
