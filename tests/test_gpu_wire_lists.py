"""GPU: the way back from the packed wire form with prefix LISTS (prf_small_unpack_lists_kernel, prf_wide_unpack_lists_kernel<BS>) through
the engine methods: float64 BYTES against codec_ref's unquantise (and ref_unbatch) of the CPU oracle's decrypt with the same lists, the
sums from codec_ref.sum_plane (slots carry and wrap) under the inverse mask.  Outputs are filled with 0xFF, a guard value behind them."""
import numpy as np
import pytest

import codec_ref as R
import test_gpu_wire_batched as B
import wire_ref as W
from test_gpu_wire_batched import orc  # noqa: F401  (the oracle fixture)
from wire_ref import C, EBITS, GUARD, IT, KEY

pytestmark = pytest.mark.gpu

# paired, an odd tail, add-only, minus-only, unequal, a repeated prefix (the single mask sums duplicates)
LISTS = (([2, 5], [0, 3]), ([2, 5, 8], [0, 3, 6]), ([], [0, 1, 2]), ([1, 4, 7], []), ([2, 5], [0]), ([], [0, 0, 1]))
FULL = (list(range(1, 192, 2)), list(range(0, 192, 2)))              # 96 + 96: lanes of three waves fill the table


@pytest.fixture(scope="module")
def engines():
    from flashe_amd.engine import Engine
    made = {}
    return lambda b: made.setdefault(b, Engine(KEY, b, device=0))


def _check(orc, eng, call, pt, n, b, add, minus, n_jobs, n_values, floats_of):
    """pt under the inverse mask through `call`: the bytes of floats_of(the oracle's decrypt with the lists), the guard untouched."""
    ct = orc.decrypt(KEY, IT, minus, add, n_jobs, b, orc.ints_to_limbs(pt, b))
    floats = floats_of(orc.limbs_to_ints(orc.decrypt(KEY, IT, add, minus, n_jobs, b, ct)))
    out = eng.alloc(8 * (n_values + 1))
    eng.memset_dev(out, 0xFF, out.nbytes)
    tag = (b, add[:4], minus[:4], n_jobs, n)
    assert call(eng.upload(W.int_limbs(W.wire_int(orc.limbs_to_ints(ct), b), W.n_limbs_of(n, b))), out), tag
    res = out.download(np.uint64, n_values + 1)
    assert int(res[n_values]) == GUARD, ("guard value",) + tag
    assert res[:n_values].tobytes() == floats.tobytes(), tag + (np.flatnonzero(res[:n_values] != floats.view(np.uint64))[:4],)


def _dense(eng, orc, b, add, minus, n_jobs, n):
    model = W.three_layer_model(n)                                    # three rows: a tile straddles a row
    plane = R.sum_plane(EBITS, C, int_bits=b, n_random=500)
    back = [(s, None, a, False) for s, a in zip(model.starts, model.alphas)]
    _check(orc, eng, lambda din, out: eng.unpack_decrypt_lists_unquantize_model_dev(IT, add, minus, n, n_jobs, din, back, EBITS, C, out),
           [plane[j % len(plane)] % (1 << b) for j in range(n)], n, b, add, minus, n_jobs, n,
           lambda dec: W.row_floats(dec, model.starts, model.sizes, model.alphas))


def _batched(eng, orc, b, fb, add, minus, n):
    bs, ebits = b // fb, fb - 2
    _xs, sizes, elems, _u = B._model(bs, n)
    plane = R.sum_plane(ebits, C, int_bits=fb, n_random=500)
    vals = [[plane[(s + j) % len(plane)] for j in range(sz)] for s, sz in zip(B._starts(sizes), sizes)]
    rows = [(sz, None, a, False) for sz, a in zip(sizes, B.ALPHAS)]
    _check(orc, eng, lambda din, out: eng.unpack_decrypt_lists_unbatch_unquantize_model_dev(IT, add, minus, rows, ebits, fb, C, din, n, out),
           [t % (1 << b) for v in vals for t in R.ref_batch(v, b, fb)], n, b, add, minus, 1, sum(sizes),
           lambda dec: np.concatenate([R.ref_unquantize(R.ref_unbatch(dec[es:es + ne], b, fb)[:sz], a, ebits, C)
                                       for es, ne, sz, a in zip(B._starts(elems), elems, sizes, B.ALPHAS)]))


@pytest.mark.parametrize("add,minus", LISTS)
@pytest.mark.parametrize("b", [16, 20, 23, 32, 33, 64])
def test_dense_lists_match_the_oracle_as_float64_bytes(engines, orc, b, add, minus):
    m = 128 // b
    for n_jobs in (1, 16):
        for n in (1, 64 * m - 1, 3 * 64 * m + 7):                     # a ragged-only tile; one short tile; whole tiles and a ragged one
            _dense(engines(b), orc, b, add, minus, n_jobs, n)


@pytest.mark.parametrize("add,minus", LISTS)
@pytest.mark.parametrize("b,fb", B.WIDTHS)
def test_batched_lists_match_the_oracle_as_float64_bytes(engines, orc, b, fb, add, minus):
    for n in B.N_ELEMS:
        _batched(engines(b), orc, b, fb, add, minus, n)


@pytest.mark.parametrize("b,fb", [(20, 0), (64, 0), (120, 20)])
def test_the_full_table_decrypts_and_a_longer_list_is_declined_untouched(engines, orc, b, fb):
    eng, n, bs = engines(b), 100, (b // fb if fb else 1)
    _batched(eng, orc, b, fb, *FULL, 1) if fb else _dense(eng, orc, b, *FULL, 1, 1)
    packed, out = eng.alloc(8 * W.n_limbs_of(n, b)), eng.alloc(8 * n * bs)
    for buf in (packed, out):
        eng.memset_dev(buf, 0xFF, buf.nbytes)
    for lists, add in (("lists_", list(range(97))), ("", [5, 9])):      # 97 + 1 above the cap; 2 + 1 at the one-prefix entry points
        if fb:
            assert not getattr(eng, f"unpack_decrypt_{lists}unbatch_unquantize_model_dev")(IT, add, [4], [(n * bs, None, 1.0, False)], fb - 2, fb, C, packed, n, out)
        else:
            assert not getattr(eng, f"unpack_decrypt_{lists}unquantize_model_dev")(IT, add, [4], n, 1, packed, [(0, None, 1.0, False)], EBITS, C, out)
    for buf in (packed, out):
        assert (buf.download(np.uint8, buf.nbytes) == 0xFF).all(), (b, fb)
