"""GPU: the one-limb cohort's chained launch for a round in which clients dropped out (flashe_quantize_encrypt_cohort_runs_u64_dev;
prf_limb_cohort_runs_kernel<2 | 3>, int_bits 33 .. 64) against the NumPy reference of tests/codec_ref.py composed with the oracle's cipher at
the gapped indices -- no other kernel of this engine takes part.  Every ciphertext is the oracle's double-mask encrypt of ref_quantize's
plaintext at that client's own index, the sum is the oracle's, and the oracle's decrypt of that sum with telescope(idx) gives the sum of
the plaintexts (no mask is written at these widths).  The models are those of tests/test_gpu_cohort_edges.py's compact chain at the lengths
of tests/test_gpu_cohort_limb.py: odd lengths a few hundred values past the admission on two CUs, chunks that end in partial blocks, so
tiles walk and row boundaries fall inside half tiles; client 1's outputs lie 8 bytes past a 16-byte boundary; one index set ends at
2^32 - 2.  Outputs are poisoned with 0xA5 and one guard element behind each must stay so; a refused call leaves all of them untouched.  One
case of 40 clients in 32 runs (72 streams: the link lookup past its first sixteen-stream word and past its first base word) against the
engine's own per-client fused step, and the 144-stream boundary with every client reading one model.  Integers are compared exactly: no
tolerance anywhere."""
import functools

import numpy as np
import pytest

import codec_ref as R
from test_gpu_cohort_compact_dropout_edges import _many_idx
from test_gpu_cohort_dropout_edges import INDEX_SETS
from test_gpu_cohort_edges import C, IT, KEY, _get, _ints, _limbs, _out, _same, _sources, _want_cts, compact_spec
from test_gpu_cohort_limb import _length

pytestmark = pytest.mark.gpu

TOP = 2 ** 32
# int_bits, element_bits: both M (3 up to 42, 2 from 43), the switch at 42 | 43, element_bits == int_bits (q == 2^bits wraps to 0), slots
# that straddle the 64-bit halves, the full-width mask, float64's 52 | 53 bits
WIDTHS = [(33, 29), (33, 33), (40, 32), (42, 38), (42, 42), (43, 39), (48, 40), (63, 59), (64, 60), (64, 52), (64, 53)]
CASES = [(b, bits, 16, "one-gap") for b, bits in WIDTHS] + \
        [(b, bits, J, name) for b, bits in ((40, 32), (64, 60)) for J in (1, 16) for name in INDEX_SETS if (J, name) != (16, "one-gap")]


@pytest.fixture(scope="module")
def E():
    from flashe_amd import engine
    return engine


def limb_length(b, J):
    """An odd length a few hundred values past the one-limb launch's admission on two CUs (test_gpu_cohort_limb._length): odd, so that
    client 1's draws begin at an address that is 8 mod 16."""
    for extra in range(300, 600):
        n = _length(b, J, extra=extra)
        if n % 2:
            return n
    raise AssertionError((b, J))


@functools.lru_cache(maxsize=None)
def _case(b, bits, J):
    model = R.cohort_model(compact_spec(limb_length(b, J)), C, seed=b + bits + J)
    return model, [[int(v) for v in p] for p in R.check_cohort_case(model, bits)]


def _launch(E, eng, model, call):
    """-> what the call answered, the C ciphertexts and the sum as Python ints, every guard"""
    n = model.n
    srcs, dts, keep = _sources(eng, model, odd_client=1)
    du = eng.upload(model.u)
    outs = [_out(E, eng, n, 8, off=8 if c == 1 else 0) for c in range(C + 1)]
    ok = call(srcs, dts, du, outs[:C], outs[C])
    got = [_get(d, n, 8) for d in outs]
    del keep
    return ok, [g for g, _guard in got], [guard for _g, guard in got]


@pytest.mark.parametrize("b,bits,J,name", CASES)
def test_the_gapped_one_limb_chain_against_numpy_and_the_oracle(E, oracle, b, bits, J, name):
    model, pts = _case(b, bits, J)
    idx = INDEX_SETS[name]
    n, M = model.n, (1 << b) - 1
    assert n % 2 == 1
    eng = E.Engine(KEY, b, device=0)
    eng.set_cu_limit(2)
    what = ("gapped one-limb chain", b, bits, J, name)
    ok, got, guards = _launch(E, eng, model, lambda srcs, dts, du, cts, dsum:
                              eng.quantize_encrypt_cohort_runs_u64_dev(IT, idx, n, J, model.rows, srcs, dts, bits, du, cts, dsum))
    assert ok, ("the chained launch declined the shape", what)
    assert all(guards), ("a write behind an output", what, guards)
    want, want_sum = _want_cts(oracle, pts, b, J, idx=idx)
    for c in range(C):
        _same(got[c], want[c], what, "client", c, "index", idx[c])
    _same(got[C], want_sum, what, "sum")
    add, minus = oracle.telescope(list(idx))
    dec = _ints(oracle.decrypt(KEY, IT, add, minus, J, b, _limbs([int(v) for v in got[C]], b)))
    _same(dec, np.array([sum(t) & M for t in zip(*pts)], dtype=object), what, "the oracle's decrypt of the sum with telescope(idx)")
    if name == "one-run":
        ok, old, guards = _launch(E, eng, model, lambda srcs, dts, du, cts, dsum:
                                  eng.quantize_encrypt_cohort_u64_dev(IT, idx[0], n, J, model.rows, srcs, dts, bits, du, cts, dsum))
        assert ok and all(guards)
        for c in range(C + 1):
            _same(got[c], old[c], what, "the bytes of quantize_encrypt_cohort_u64_dev", c)


# ------------------------------------------------------------------------------------------------ many streams
@pytest.mark.parametrize("b,bits", [(40, 32), (64, 60)])
def test_forty_clients_in_thirty_two_runs_against_the_per_client_step(E, b, bits):
    """Streams 16 .. 71 find their links through the second to fifth word of the stream bits and the second base word.  The reference is
    quantize_encrypt_model_dev of every client at its own index on the same engine (itself checked against the oracle by
    tests/test_gpu_codec_fused.py), compared as integers, and NumPy for the sum."""
    from flashe_amd import _lib
    from flashe_amd.block import compact_cohort_admission_length
    from flashe_amd.engine import SCHEME_DOUBLE
    idx, J = _many_idx(), 16
    nc = len(idx)
    runs = 1 + sum(1 for a, z in zip(idx, idx[1:]) if z != a + 1)
    assert nc == 40 and nc + runs == 72
    n = compact_cohort_admission_length(2, b, J) + 301
    sizes = [1001, n - 1001]
    alphas = [0.5, 2.0]
    rng = np.random.Generator(np.random.PCG64(40 + b))
    eng = E.Engine(KEY, b, device=0)
    eng.set_cu_limit(2)
    du = eng.upload(rng.random(nc * n))
    xs = [[eng.upload(rng.uniform(-1.2 * a, 1.2 * a, s).astype(np.float32)) for s, a in zip(sizes, alphas)] for _c in range(nc)]
    rows = [(0, None, alphas[0], 0.0, _lib.TENSOR_F32, 0), (sizes[0], None, alphas[1], 0.0, _lib.TENSOR_F32, 0)]
    outs = [_out(E, eng, n, 8) for _ in range(nc + 1)]
    assert eng.quantize_encrypt_cohort_runs_u64_dev(IT, idx, n, J, rows, [[x.ptr for x in row] for row in xs], [[_lib.TENSOR_F32] * 2] * nc,
                                                    bits, du, outs[:nc], outs[nc]), "the chained launch declined the shape"
    ref = eng.alloc(8 * n)
    total = np.zeros(n, dtype=np.uint64)
    for c in range(nc):
        layers = [(0, xs[c][0].ptr, alphas[0], False), (sizes[0], xs[c][1].ptr, alphas[1], False)]
        eng.quantize_encrypt_model_dev(IT, idx[c], SCHEME_DOUBLE, n, J, 0, n, layers, bits, E.DeviceBufferView(du, 8 * c * n, 8 * n), ref)
        want = ref.download(np.uint64, n)
        total += want
        got = outs[c].download(np.uint64, n + 1)
        assert got[n] == np.uint64(0xA5A5A5A5A5A5A5A5), ("a write behind the ciphertext", c)
        assert np.array_equal(got[:n], want), ("client", c, "index", idx[c], np.flatnonzero(got[:n] != want)[:6])
    got = outs[nc].download(np.uint64, n + 1)
    assert got[n] == np.uint64(0xA5A5A5A5A5A5A5A5), "a write behind the sum"
    assert np.array_equal(got[:n], total & np.uint64((1 << b) - 1)), "sum"


# ------------------------------------------------------------------------------------------------ the stream boundary and the refusals
def _one_model_cohort(eng, n_clients, n, width=8, seed=None):
    """Clients that all read client 0's model (zeros without a seed) and its draws' neighbours; poisoned outputs of `width` bytes per
    element.  -> rows, srcs, dts, draws, outputs, the model's device buffer"""
    from flashe_amd import _lib
    g = np.random.Generator(np.random.PCG64(seed or 0))
    x = eng.upload(g.uniform(-1.1, 1.1, n).astype(np.float32) if seed else np.zeros(n, np.float32))
    du = eng.upload(g.random(n_clients * n) if seed else np.zeros(n_clients * n))
    outs = [eng.alloc(width * n) for _ in range(n_clients + 1)]
    for d in outs:
        eng.memset_dev(d, 0xA5, width * n)
    rows = [(0, None, 1.0, 0.0, _lib.TENSOR_F32, 0)]
    return rows, [[x.ptr]] * n_clients, [[_lib.TENSOR_F32]] * n_clients, du, outs, x


def _untouched(outs, n, width=8):
    return all((d.download(np.uint64, n * width // 8) == np.uint64(0xA5A5A5A5A5A5A5A5)).all() for d in outs)


def _runs_of(n_clients, runs):
    """n_clients cipher indices from 3 on in `runs` runs: a gap of one index in front of each run but the first."""
    per = n_clients // runs
    return [3 + c + min(c // per, runs - 1) for c in range(n_clients)]


def test_128_clients_in_16_runs_chain_and_match(E):
    """144 streams, the table's last prefix slot.  Every client reads client 0's model (as test_the_link_table_boundary does) with its own
    draws; the reference is quantize_encrypt_model_dev per client at its own index, and NumPy for the sum."""
    from flashe_amd.block import compact_cohort_admission_length
    from flashe_amd.engine import SCHEME_DOUBLE
    b, bits, J, nc = 40, 32, 16, 128
    idx = _runs_of(nc, 16)
    assert len(idx) == nc and nc + 1 + sum(1 for a, z in zip(idx, idx[1:]) if z != a + 1) == 144
    n = compact_cohort_admission_length(2, b, J) + 301
    eng = E.Engine(KEY, b, device=0)
    eng.set_cu_limit(2)
    rows, srcs, dts, du, outs, x = _one_model_cohort(eng, nc, n, seed=7)
    assert eng.quantize_encrypt_cohort_runs_u64_dev(IT, idx, n, J, rows, srcs, dts, bits, du, outs[:nc], outs[nc]), "the chained launch declined the shape"
    ref = eng.alloc(8 * n)
    total = np.zeros(n, dtype=np.uint64)
    for c in range(nc):
        eng.quantize_encrypt_model_dev(IT, idx[c], SCHEME_DOUBLE, n, J, 0, n, [(0, x.ptr, 1.0, False)], bits, E.DeviceBufferView(du, 8 * c * n, 8 * n), ref)
        want = ref.download(np.uint64, n)
        total += want
        got = outs[c].download(np.uint64, n)
        assert np.array_equal(got, want), ("client", c, "index", idx[c], np.flatnonzero(got != want)[:6])
    assert np.array_equal(outs[nc].download(np.uint64, n), total & np.uint64((1 << b) - 1)), "sum"


@pytest.mark.parametrize("nc,runs", [(128, 17), (73, 73)], ids=["145-streams", "146-streams"])
def test_more_than_144_streams_are_declined_with_every_output_untouched(E, nc, runs):
    from flashe_amd.block import compact_cohort_admission_length
    n = compact_cohort_admission_length(2, 40, 16)
    eng = E.Engine(KEY, 40, device=0)
    eng.set_cu_limit(2)
    rows, srcs, dts, du, outs, _x = _one_model_cohort(eng, nc, n)
    idx = _runs_of(nc, runs)
    assert nc + 1 + sum(1 for a, z in zip(idx, idx[1:]) if z != a + 1) == nc + runs > 144
    assert eng.quantize_encrypt_cohort_runs_u64_dev(IT, idx, n, 16, rows, srcs, dts, 32, du, outs[:nc], outs[nc]) is False
    assert _untouched(outs, n)


@pytest.mark.parametrize("idx", [[5, 8, 6], [5, 5, 6], [5, 6, TOP - 1]], ids=["unsorted", "repeated", "top"])
def test_bad_indices_are_einval_and_leave_the_outputs_untouched(E, idx):
    from flashe_amd.block import compact_cohort_admission_length
    n = compact_cohort_admission_length(2, 40, 16)
    eng = E.Engine(KEY, 40, device=0)
    eng.set_cu_limit(2)
    rows, srcs, dts, du, outs, _x = _one_model_cohort(eng, 3, n)
    with pytest.raises(E.FlasheError) as ei:
        eng.quantize_encrypt_cohort_runs_u64_dev(IT, idx, n, 16, rows, srcs, dts, 32, du, outs[:3], outs[3])
    assert ei.value.code == -22
    assert _untouched(outs, n)
    for bad in ([5, 6, TOP], [-1, 5, 6], [5, 6]):              # nothing is reduced mod 2^32 or cut on the way to the library
        with pytest.raises(ValueError):
            eng.quantize_encrypt_cohort_runs_u64_dev(IT, bad, n, 16, rows, srcs, dts, 32, du, outs[:3], outs[3])
    assert _untouched(outs, n)


@pytest.mark.parametrize("b,bits", [(40, 32), (64, 60)])
def test_one_value_below_admission_is_declined_untouched(E, b, bits):
    from flashe_amd.block import compact_cohort_admission_length
    n = compact_cohort_admission_length(2, b, 16)
    eng = E.Engine(KEY, b, device=0)
    eng.set_cu_limit(2)
    rows, srcs, dts, du, outs, _x = _one_model_cohort(eng, 3, n)
    assert eng.quantize_encrypt_cohort_runs_u64_dev(IT, [5, 6, 8], n - 1, 16, rows, srcs, dts, bits, du, outs[:3], outs[3]) is False
    assert _untouched(outs, n)
    assert eng.quantize_encrypt_cohort_runs_u64_dev(IT, [5, 6, 8], n, 16, rows, srcs, dts, bits, du, outs[:3], outs[3]) is True


@pytest.mark.parametrize("b,bits", [(32, 24), (65, 60)])
def test_a_ctx_of_another_width_declines_untouched(E, b, bits):
    """(a two-limb ctx: 16 bytes per element, so that only the width stands against the launch)"""
    n = _length(33, 16, extra=5000)
    eng = E.Engine(KEY, b, device=0)
    eng.set_cu_limit(2)
    rows, srcs, dts, du, outs, _x = _one_model_cohort(eng, 3, n, width=16)
    assert eng.quantize_encrypt_cohort_runs_u64_dev(IT, [5, 6, 8], n, 16, rows, srcs, dts, bits, du, outs[:3], outs[3]) is False
    assert _untouched(outs, n, width=16)
