"""GPU: the cohort's chained launches for a round in which clients dropped out (flashe_quantize_encrypt_cohort_runs_dev,
flashe_quantize_batch_encrypt_cohort_runs_dev; prf_chain_cohort_runs_kernel and prf_chain_cohort_batch_runs_kernel<1024, 5 / 6 / 7>) against
the NumPy / Python-int reference of tests/codec_ref.py composed with the oracle's cipher at the gapped indices -- no other kernel of this
engine takes part.  Every ciphertext is the oracle's double-mask encrypt of ref_quantize / ref_batch's plaintext at that client's index,
the sum is the Python-int sum, and the decrypt mask is the oracle's terms of telescope(P): + one past every run's end, - every run's start.
The models are those of tests/test_gpu_cohort_edges.py: q == 2^bits (and the carry into the neighbouring field and out of a 120-bit
element where field_bits == element_bits), row boundaries inside a pair of a tile, a staged 16-bit row; client 1's outputs lie one
element past a 16-byte boundary; one index set ends at 2^32 - 2.  Two CUs, a few hundred elements past the admission length.  Outputs are
poisoned with 0xA5 and one guard element behind each must stay so; a refused call leaves all of them untouched.  Integers are compared
exactly: no tolerance anywhere."""
import functools

import numpy as np
import pytest

import codec_ref as R
from test_gpu_cohort_edges import CHAIN_ELEMS, IT, KEY, _get, _ints, _limbs, _out, _same, _sources, batch_case, prepared_spec

pytestmark = pytest.mark.gpu

C, J = 3, 16
TOP = 2 ** 32
# the cipher indices of the three clients that report
INDEX_SETS = {
    "one-gap": [5, 6, 8],                       # stream 7 closes client 6 and opens none, stream 8 opens and closes none
    "every-other": [5, 7, 9],                   # every stream is a run boundary
    "skipped-streams": [5, 9, 10],              # streams 7 and 8 lie inside a dropped run and are not computed
    "one-run": [3, 4, 5],                       # the kernels of flashe_quantize_encrypt_cohort_dev
    "top": [TOP - 5, TOP - 4, TOP - 2],         # the last stream is 2^32 - 1
}
PLAIN = [(128, 24), (120, 62)]                                  # int_bits, element_bits
BATCHED = [(120, 24, 24), (120, 20, 20), (128, 18, 18)]         # int_bits, field_bits, element_bits: bs 5, 6, 7 with carries


@pytest.fixture(scope="module")
def E():
    from flashe_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def plain_case(b, bits):
    model = R.cohort_model(prepared_spec(CHAIN_ELEMS), C, seed=b + bits)
    pts = R.check_cohort_case(model, bits)
    return model, [[int(v) for v in p] for p in pts]


@functools.lru_cache(maxsize=None)
def batched_case(b, fb, eb):
    model, _pts, batched, _over = batch_case(b, fb, eb, CHAIN_ELEMS)
    return model, batched


def _want(oracle, pts, b, idx):
    """Every present client's oracle ciphertext at its own index, their Python-int sum, and the mask of the telescoped lists."""
    M = (1 << b) - 1
    n = len(pts[0])
    cts = [_ints(oracle.encrypt(KEY, IT, idx[c], "double", J, b, _limbs([v & M for v in p], b))) for c, p in enumerate(pts)]
    total = np.array([sum(t) & M for t in zip(*cts)], dtype=object)
    add, minus = oracle.telescope(list(idx))
    D = np.zeros(n, dtype=object)
    for i in add:
        D = D + _ints(oracle.mask(KEY, IT, i, n, J, b))
    for i in minus:
        D = D - _ints(oracle.mask(KEY, IT, i, n, J, b))
    plain = np.array([sum(t) & M for t in zip(*pts)], dtype=object)
    return cts, total, D & M, plain


def _launch(E, eng, model, idx, ne, call, dmask=True):
    srcs, dts, keep = _sources(eng, model, odd_client=1)
    du = eng.upload(model.u)
    outs = [_out(E, eng, ne, 16, off=16 if c == 1 else 0) for c in range(C + 2)]
    ok = call(srcs, dts, du, outs[:C], outs[C], outs[C + 1] if dmask else None)
    got = [_get(d, ne, 16) for d in outs]
    del keep
    return ok, [g for g, _guard in got], [guard for _g, guard in got]


def _check(E, oracle, eng, model, pts, b, idx, ne, call, what):
    M = (1 << b) - 1
    ok, got, guards = _launch(E, eng, model, idx, ne, call)
    assert ok, ("the chained launch declined the shape", what)
    assert all(guards), ("a write behind an output", what, guards)
    cts, total, D, plain = _want(oracle, pts, b, idx)
    for c in range(C):
        _same(got[c], cts[c], what, "client", c, "index", idx[c])
    _same(got[C], total, what, "sum")
    _same(got[C + 1], D, what, "decrypt mask against the oracle's terms of telescope(P)")
    _same((got[C] + got[C + 1]) & M, plain, what, "sum + mask against the NumPy plaintexts")


@pytest.mark.parametrize("name", list(INDEX_SETS))
@pytest.mark.parametrize("b,bits", PLAIN)
def test_the_gapped_chain_against_numpy_and_the_oracle(E, oracle, b, bits, name):
    model, pts = plain_case(b, bits)
    idx = INDEX_SETS[name]
    eng = E.Engine(KEY, b, device=0)
    eng.set_cu_limit(2)

    def call(srcs, dts, du, cts, dsum, dmask):
        return eng.quantize_encrypt_cohort_runs_dev(IT, idx, model.n, J, model.rows, srcs, dts, bits, du, cts, dsum, dmask)
    _check(E, oracle, eng, model, pts, b, idx, model.n, call, ("un-batched", b, bits, name))


@pytest.mark.parametrize("name", list(INDEX_SETS))
@pytest.mark.parametrize("b,fb,eb", BATCHED)
def test_the_gapped_batched_chain_against_numpy_and_the_oracle(E, oracle, b, fb, eb, name):
    model, batched = batched_case(b, fb, eb)
    idx = INDEX_SETS[name]
    eng = E.Engine(KEY, b, device=0)
    eng.set_cu_limit(2)

    def call(srcs, dts, du, cts, dsum, dmask):
        return eng.quantize_batch_encrypt_cohort_runs_dev(IT, idx, model.n, CHAIN_ELEMS, J, model.rows, srcs, dts, eb, fb, du, cts, dsum, dmask)
    _check(E, oracle, eng, model, batched, b, idx, CHAIN_ELEMS, call, ("batched", b, fb, eb, name))


def test_without_a_mask_the_other_outputs_are_the_same(E, oracle):
    model, pts = plain_case(128, 24)
    idx = INDEX_SETS["one-gap"]
    eng = E.Engine(KEY, 128, device=0)
    eng.set_cu_limit(2)

    def call(srcs, dts, du, cts, dsum, dmask):
        return eng.quantize_encrypt_cohort_runs_dev(IT, idx, model.n, J, model.rows, srcs, dts, 24, du, cts, dsum, dmask)
    ok, got, guards = _launch(E, eng, model, idx, model.n, call, dmask=False)
    assert ok and all(guards)
    cts, total, _D, _plain = _want(oracle, pts, 128, idx)
    for c in range(C):
        _same(got[c], cts[c], "no mask", "client", c)
    _same(got[C], total, "no mask", "sum")
    assert all(int(v) == 0xA5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5 for v in got[C + 1]), "the mask vector was written"


# ------------------------------------------------------------------------------------------------ refusals
def _zero_cohort(E, eng, n_clients, n_values, n_out):
    """Clients that all read one zero model; poisoned outputs.  -> rows, srcs, dts, draws, outputs"""
    from flashe_amd import _lib
    x = eng.upload(np.zeros(n_values, np.float32))
    du = eng.upload(np.zeros(n_clients * n_values))
    outs = [eng.alloc(16 * n_out) for _ in range(n_clients + 2)]
    for d in outs:
        eng.memset_dev(d, 0xA5, 16 * n_out)
    rows = [(0, None, 1.0, 0.0, _lib.TENSOR_F32, 0)]
    return rows, [[x.ptr]] * n_clients, [[_lib.TENSOR_F32]] * n_clients, du, outs


def _untouched(outs, n_out):
    return all((d.download(np.uint64, 2 * n_out) == np.uint64(0xA5A5A5A5A5A5A5A5)).all() for d in outs)


@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("idx", [[5, 8, 6], [5, 5, 6], [5, 6, TOP - 1], [TOP - 1, 0, 1]], ids=["unsorted", "duplicate", "top", "wrapped"])
def test_bad_indices_are_einval_and_leave_the_outputs_untouched(E, batched, idx):
    b = 120 if batched else 128
    eng = E.Engine(KEY, b, device=0)
    eng.set_cu_limit(2)
    ne = CHAIN_ELEMS
    n = 6 * ne if batched else ne
    rows, srcs, dts, du, outs = _zero_cohort(E, eng, 3, n, ne)
    with pytest.raises(E.FlasheError) as ei:
        if batched:
            eng.quantize_batch_encrypt_cohort_runs_dev(IT, idx, n, ne, J, rows, srcs, dts, 16, 20, du, outs[:3], outs[3], outs[4])
        else:
            eng.quantize_encrypt_cohort_runs_dev(IT, idx, n, J, rows, srcs, dts, 16, du, outs[:3], outs[3], outs[4])
    assert ei.value.code == -22
    assert _untouched(outs, ne)
    for bad in ([5, 6, TOP], [-1, 5, 6], [5, 6]):              # nothing is reduced mod 2^32 or cut on the way to the library
        with pytest.raises(ValueError):
            eng.quantize_encrypt_cohort_runs_dev(IT, bad, n, J, rows, srcs, dts, 16, du, outs[:3], outs[3], outs[4])
    assert _untouched(outs, ne)


def test_shapes_outside_the_launch_are_enotsup_and_leave_the_outputs_untouched(E):
    from flashe_amd.block import cohort_admission_length
    adm = cohort_admission_length(2)
    eng = E.Engine(KEY, 128, device=0)
    eng.set_cu_limit(2)
    # one run too many: 73 singletons need 146 streams (72 fit: 144)
    for n_clients, took in ((72, True), (73, False)):
        rows, srcs, dts, du, outs = _zero_cohort(E, eng, n_clients, adm, adm)
        idx = list(range(0, 2 * n_clients, 2))
        ok = eng.quantize_encrypt_cohort_runs_dev(IT, idx, adm, J, rows, srcs, dts, 16, du, outs[:n_clients], outs[n_clients], outs[n_clients + 1])
        assert ok is took
        assert _untouched(outs, adm) is (not took)
    # a vector one element short of the admission length
    rows, srcs, dts, du, outs = _zero_cohort(E, eng, 3, adm - 1, adm - 1)
    assert eng.quantize_encrypt_cohort_runs_dev(IT, [5, 6, 8], adm - 1, J, rows, srcs, dts, 16, du, outs[:3], outs[3], outs[4]) is False
    assert _untouched(outs, adm - 1)
    # int_bits 64
    eng64 = E.Engine(KEY, 64, device=0)
    eng64.set_cu_limit(2)
    rows, srcs, dts, du, outs = _zero_cohort(E, eng64, 3, adm, adm)
    assert eng64.quantize_encrypt_cohort_runs_dev(IT, [5, 6, 8], adm, J, rows, srcs, dts, 16, du, outs[:3], outs[3], outs[4]) is False
    assert _untouched(outs, adm)
    # four values per element (field_bits 30 at int_bits 120), and one batched element short
    eng120 = E.Engine(KEY, 120, device=0)
    eng120.set_cu_limit(2)
    rows, srcs, dts, du, outs = _zero_cohort(E, eng120, 3, 4 * adm, adm)
    assert eng120.quantize_batch_encrypt_cohort_runs_dev(IT, [5, 6, 8], 4 * adm, adm, J, rows, srcs, dts, 16, 30, du, outs[:3], outs[3], outs[4]) is False
    assert _untouched(outs, adm)
    rows, srcs, dts, du, outs = _zero_cohort(E, eng120, 3, 6 * (adm - 1), adm - 1)
    assert eng120.quantize_batch_encrypt_cohort_runs_dev(IT, [5, 6, 8], 6 * (adm - 1), adm - 1, J, rows, srcs, dts, 16, 20, du, outs[:3], outs[3],
                                                         outs[4]) is False
    assert _untouched(outs, adm - 1)
