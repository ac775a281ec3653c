"""GPU: the compact cohort's chained launch for a round in which clients dropped out (flashe_quantize_encrypt_cohort_runs_u32_dev;
prf_small_cohort_runs_kernel<16 / 20 / 23 / 24 / 32>) against the NumPy reference of tests/codec_ref.py composed with the oracle's cipher at
the gapped indices -- no other kernel of this engine takes part.  Every ciphertext is the oracle's double-mask encrypt of ref_quantize's
plaintext at that client's own index, the sum is the oracle's, and the oracle's decrypt of that sum with telescope(idx) gives the sum of
the plaintexts (no mask is written at these widths).  The models and lengths are those of tests/test_gpu_cohort_edges.py's compact chain:
odd lengths a few hundred values past the admission on two CUs, every chunk ends in a partial block, so tiles walk and row boundaries
fall inside half tiles; client 1's outputs lie 4 bytes past a 16-byte boundary; one index set ends at 2^32 - 2.  Outputs are poisoned with
0xA5 and one guard element behind each must stay so; a refused call leaves all of them untouched.  One case of 40 clients in 32 runs (72
streams: the link lookup past its first sixteen-stream word and past its first base word) against the engine's own per-client fused step.
Integers are compared exactly: no tolerance anywhere."""
import functools

import numpy as np
import pytest

import codec_ref as R
from test_gpu_cohort_dropout_edges import INDEX_SETS
from test_gpu_cohort_edges import C, IT, KEY, _get, _ints, _limbs, _out, _same, _sources, _want_cts, compact_case

pytestmark = pytest.mark.gpu

TOP = 2 ** 32
WIDTHS = [(16, 16), (20, 20), (23, 23), (24, 24), (32, 32), (32, 25)]                     # int_bits, element_bits: every width once, "one-gap", J = 16
CASES = [(b, bits, 16, "one-gap") for b, bits in WIDTHS] + [(20, 20, J, name) for J in (1, 16) for name in INDEX_SETS if (J, name) != (16, "one-gap")]


@pytest.fixture(scope="module")
def E():
    from flashe_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def _case(b, bits, J):
    model, pts = compact_case(b, bits, J)
    return model, [[int(v) for v in p] for p in pts]


def _launch(E, eng, model, call):
    """-> what the call answered, the C ciphertexts and the sum as Python ints, every guard"""
    n = model.n
    srcs, dts, keep = _sources(eng, model, odd_client=1)
    du = eng.upload(model.u)
    outs = [_out(E, eng, n, 4, off=4 if c == 1 else 0) for c in range(C + 1)]
    ok = call(srcs, dts, du, outs[:C], outs[C])
    got = [_get(d, n, 4) for d in outs]
    del keep
    return ok, [g for g, _guard in got], [guard for _g, guard in got]


@pytest.mark.parametrize("b,bits,J,name", CASES)
def test_the_gapped_compact_chain_against_numpy_and_the_oracle(E, oracle, b, bits, J, name):
    model, pts = _case(b, bits, J)
    idx = INDEX_SETS[name]
    n, M = model.n, (1 << b) - 1
    assert n % 2 == 1
    eng = E.Engine(KEY, b, device=0)
    eng.set_cu_limit(2)
    what = ("gapped compact chain", b, bits, J, name)
    ok, got, guards = _launch(E, eng, model, lambda srcs, dts, du, cts, dsum:
                              eng.quantize_encrypt_cohort_runs_u32_dev(IT, idx, n, J, model.rows, srcs, dts, bits, du, cts, dsum))
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
                                  eng.quantize_encrypt_cohort_u32_dev(IT, idx[0], n, J, model.rows, srcs, dts, bits, du, cts, dsum))
        assert ok and all(guards)
        for c in range(C + 1):
            _same(got[c], old[c], what, "the bytes of quantize_encrypt_cohort_u32_dev", c)


# ------------------------------------------------------------------------------------------------ many streams
MANY_B, MANY_BITS, MANY_J = 20, 16, 16


def _many_idx():
    """40 clients as eight groups of a pair and three singletons: 32 runs, 72 streams."""
    idx, at = [], 3
    for _g in range(8):
        idx += [at, at + 1, at + 3, at + 5, at + 7]
        at += 9
    return idx


def test_forty_clients_in_thirty_two_runs_against_the_per_client_step(E):
    """Streams 16 .. 71 find their links through the second to fifth word of the stream bits and the second base word.  The reference is
    quantize_encrypt_model_dev of every client at its own index on the same engine (itself checked against the oracle by
    tests/test_gpu_codec_fused.py), compared as integers."""
    from flashe_amd import _lib
    from flashe_amd.block import compact_cohort_admission_length
    from flashe_amd.engine import SCHEME_DOUBLE
    idx = _many_idx()
    nc = len(idx)
    runs = 1 + sum(1 for a, z in zip(idx, idx[1:]) if z != a + 1)
    assert nc == 40 and nc + runs == 72 >= 70
    n = compact_cohort_admission_length(2, MANY_B, MANY_J) + 301
    sizes = [1001, n - 1001]
    alphas = [0.5, 2.0]
    rng = np.random.Generator(np.random.PCG64(40))
    eng = E.Engine(KEY, MANY_B, device=0)
    eng.set_cu_limit(2)
    du = eng.upload(rng.random(nc * n))
    xs = [[eng.upload(rng.uniform(-1.2 * a, 1.2 * a, s).astype(np.float32)) for s, a in zip(sizes, alphas)] for _c in range(nc)]
    rows = [(0, None, alphas[0], 0.0, _lib.TENSOR_F32, 0), (sizes[0], None, alphas[1], 0.0, _lib.TENSOR_F32, 0)]
    outs = [_out(E, eng, n, 4) for _ in range(nc + 1)]
    assert eng.quantize_encrypt_cohort_runs_u32_dev(IT, idx, n, MANY_J, rows, [[x.ptr for x in row] for row in xs], [[_lib.TENSOR_F32] * 2] * nc,
                                                    MANY_BITS, du, outs[:nc], outs[nc]), "the chained launch declined the shape"
    ref = eng.alloc(8 * n)
    total = np.zeros(n, dtype=np.uint64)
    for c in range(nc):
        layers = [(0, xs[c][0].ptr, alphas[0], False), (sizes[0], xs[c][1].ptr, alphas[1], False)]
        eng.quantize_encrypt_model_dev(IT, idx[c], SCHEME_DOUBLE, n, MANY_J, 0, n, layers, MANY_BITS, E.DeviceBufferView(du, 8 * c * n, 8 * n), ref)
        want = ref.download(np.uint64, n)
        total += want
        got, guard = _get(outs[c], n, 4)
        assert guard, ("a write behind the ciphertext", c)
        assert np.array_equal(got.astype(np.uint64), want), ("client", c, "index", idx[c], np.flatnonzero(got.astype(np.uint64) != want)[:6])
    got, guard = _get(outs[nc], n, 4)
    assert guard, "a write behind the sum"
    assert np.array_equal(got.astype(np.uint64), total & np.uint64((1 << MANY_B) - 1)), "sum"


# ------------------------------------------------------------------------------------------------ refusals
def _zero_cohort(eng, n_clients, n):
    """Clients that all read one zero model; poisoned uint32 outputs.  -> rows, srcs, dts, draws, outputs"""
    from flashe_amd import _lib
    x = eng.upload(np.zeros(n, np.float32))
    du = eng.upload(np.zeros(n_clients * n))
    outs = [eng.alloc(4 * n) for _ in range(n_clients + 1)]
    for d in outs:
        eng.memset_dev(d, 0xA5, 4 * n)
    rows = [(0, None, 1.0, 0.0, _lib.TENSOR_F32, 0)]
    return rows, [[x.ptr]] * n_clients, [[_lib.TENSOR_F32]] * n_clients, du, outs


def _untouched(outs, n):
    return all((d.download(np.uint32, n) == np.uint32(0xA5A5A5A5)).all() for d in outs)


def test_more_than_144_streams_are_declined_with_every_output_untouched(E):
    from flashe_amd.block import compact_cohort_admission_length
    n = compact_cohort_admission_length(2, 20, 16)
    eng = E.Engine(KEY, 20, device=0)
    eng.set_cu_limit(2)
    rows, srcs, dts, du, outs = _zero_cohort(eng, 73, n)
    idx = list(range(0, 146, 2))                               # 73 singletons need 146 streams
    assert eng.quantize_encrypt_cohort_runs_u32_dev(IT, idx, n, 16, rows, srcs, dts, 16, du, outs[:73], outs[73]) is False
    assert _untouched(outs, n)
    # one value below the admission length, and an engine that is not compact at another width
    assert eng.quantize_encrypt_cohort_runs_u32_dev(IT, [5, 6, 8], n - 1, 16, rows, srcs[:3], dts[:3], 16, du, outs[:3], outs[3]) is False
    assert _untouched(outs, n)
    eng21 = E.Engine(KEY, 21, device=0)
    eng21.set_cu_limit(2)
    rows, srcs, dts, du, outs = _zero_cohort(eng21, 3, n)
    assert eng21.quantize_encrypt_cohort_runs_u32_dev(IT, [5, 6, 8], n, 16, rows, srcs, dts, 16, du, outs[:3], outs[3]) is False
    assert _untouched(outs, n)


@pytest.mark.parametrize("idx", [[5, 8, 6], [5, 5, 6], [5, 6, TOP - 1]], ids=["unsorted", "repeated", "top"])
def test_bad_indices_are_einval_and_leave_the_outputs_untouched(E, idx):
    from flashe_amd.block import compact_cohort_admission_length
    n = compact_cohort_admission_length(2, 20, 16)
    eng = E.Engine(KEY, 20, device=0)
    eng.set_cu_limit(2)
    rows, srcs, dts, du, outs = _zero_cohort(eng, 3, n)
    with pytest.raises(E.FlasheError) as ei:
        eng.quantize_encrypt_cohort_runs_u32_dev(IT, idx, n, 16, rows, srcs, dts, 16, du, outs[:3], outs[3])
    assert ei.value.code == -22
    assert _untouched(outs, n)
    for bad in ([5, 6, TOP], [-1, 5, 6], [5, 6]):              # nothing is reduced mod 2^32 or cut on the way to the library
        with pytest.raises(ValueError):
            eng.quantize_encrypt_cohort_runs_u32_dev(IT, bad, n, 16, rows, srcs, dts, 16, du, outs[:3], outs[3])
    assert _untouched(outs, n)
