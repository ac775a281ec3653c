"""GPU: the batched client step straight to and from the packed wire form at int_bits 65 .. 128 (wire_wide.hip) through the engine
methods, bit for bit.  No engine kernel goes into an expected value.  Way out: codec_ref.ref_quantize and ref_batch per row (zero pads) ->
the CPU oracle's encrypt -> wire_ref.wire_int, compared as a Python int.  Way back: float64 BYTES against ref_unquantize(ref_unbatch(the
oracle's decrypt)), the fields from codec_ref.sum_plane (high bits set).  Every output buffer is filled with 0xFF with a guard behind it."""
import functools

import numpy as np
import pytest

import codec_ref as R
import wire_ref as W
from wire_ref import C, GUARD, IDX, IT, KEY

pytestmark = pytest.mark.gpu

WIDTHS = ((65, 20), (100, 20), (120, 20), (127, 20), (120, 17), (128, 21))      # bs 3 (the generic walk), 5, 6, 6 (spare top bits), 7, 6
N_ELEMS = (1, 63, 64, 65, 129, 2 * 1024 + 37)     # a top partial tile of every kind; more tiles than one workgroup has waves
ALPHAS = (8.17121, 3e-3, 6.5, 0.1, 1.0)


@functools.lru_cache(maxsize=None)
def _model(bs, n_elems):
    """Rows (dtype, size in values) that batch into n_elems elements: a float64 row with a padded last element, a one-value row, a row
    shorter than a tile, then a float32 and (the long model) a float64 row, each padded; n_elems = 1 is the one-value row alone."""
    if n_elems == 1:
        rows = [(np.float32, 1)]
    else:
        rest = n_elems - 7
        e3 = rest if rest < 1000 else 1000
        rows = [(np.float64, bs + 2), (np.float32, 1), (np.float32, 3 * bs + 1), (np.float32, e3 * bs - 1)]
        rows += [(np.float64, (rest - e3) * bs - 2)] if rest > e3 else []
    xs = [R.layer_fill(dt, ALPHAS[l], s, seed=l) for l, (dt, s) in enumerate(rows)]
    sizes = [s for _dt, s in rows]
    elems = [(s + bs - 1) // bs for s in sizes]
    assert sum(elems) == n_elems
    return xs, sizes, elems, R.mixed_draws(sum(sizes))


def _starts(v):
    return [int(s) for s in np.concatenate([[0], np.cumsum(v)[:-1]])]


def _whole_tiles(sizes, elems, bs, l):
    """Tiles (anchored at the END of the vector) inside row l that do not hold its padded last element."""
    n, es = sum(elems), _starts(elems)[l]
    return [t for t in range(n // 64) if es <= n - 64 * (t + 1) and (n - 64 * t - es) * bs <= sizes[l]]


@pytest.fixture(scope="module")
def orc():
    from oracle import flashe_oracle
    return flashe_oracle


@pytest.fixture(scope="module")
def engines():
    from flashe_amd.engine import Engine
    return {b: Engine(KEY, b, device=0) for b in sorted({b for b, _f in WIDTHS} | {64})}


@pytest.mark.parametrize("scheme", ["single", "double"])
@pytest.mark.parametrize("b,fb", WIDTHS)
def test_way_out_matches_the_oracle_and_python_ints(engines, orc, b, fb, scheme):
    from flashe_amd.engine import SCHEME_DOUBLE, SCHEME_SINGLE
    eng, bs, ebits = engines[b], b // fb, fb - 2
    for n in N_ELEMS:
        xs, sizes, elems, u = _model(bs, n)
        if n > 2048:
            assert len(_whole_tiles(sizes, elems, bs, 3)) >= 2 and len(_whole_tiles(sizes, elems, bs, 4)) >= 2     # the wave-uniform path runs
        pt = [t % (1 << b) for x, a, s, sz in zip(xs, ALPHAS, _starts(sizes), sizes) for t in R.ref_batch(R.ref_quantize(x, a, ebits, u[s:s + sz]), b, fb)]
        want = W.wire_int(orc.limbs_to_ints(orc.encrypt(KEY, IT, IDX, scheme, 1, b, orc.ints_to_limbs(pt, b))), b)
        bufs = [eng.upload(x) for x in xs]
        rows = [(sz, buf.ptr, a, x.dtype == np.float64) for sz, buf, a, x in zip(sizes, bufs, ALPHAS, xs)]
        n_limbs = W.n_limbs_of(n, b)
        packed = eng.alloc(8 * (n_limbs + 1))
        eng.memset_dev(packed, 0xFF, packed.nbytes)
        assert eng.quantize_batch_encrypt_pack_model_dev(IT, IDX, SCHEME_DOUBLE if scheme == "double" else SCHEME_SINGLE, rows, ebits, fb, eng.upload(u), n, packed)
        got = packed.download(np.uint64, n_limbs + 1)
        assert int(got[n_limbs]) == GUARD, ("guard limb", b, fb, scheme, n)
        assert int.from_bytes(got[:n_limbs].tobytes(), "little") == want, (b, fb, scheme, n, np.flatnonzero(got[:n_limbs] != W.int_limbs(want, n_limbs))[:4])


@pytest.mark.parametrize("flags", ["add+minus", "add", "minus"])
@pytest.mark.parametrize("b,fb", WIDTHS)
def test_way_back_matches_the_oracle_as_float64_bytes(engines, orc, b, fb, flags):
    eng, bs, ebits = engines[b], b // fb, fb - 2
    add, minus = {"add+minus": ([IDX + 1], [IDX]), "add": ([IDX], []), "minus": ([], [IDX])}[flags]
    plane = R.sum_plane(ebits, C, int_bits=fb, n_random=500)
    for n in N_ELEMS:
        _xs, sizes, elems, _u = _model(bs, n)
        vals = [[plane[(s + j) % len(plane)] for j in range(sz)] for s, sz in zip(_starts(sizes), sizes)]
        pt = [t % (1 << b) for v in vals for t in R.ref_batch(v, b, fb)]
        ct = orc.decrypt(KEY, IT, minus, add, 1, b, orc.ints_to_limbs(pt, b))                   # the inverse mask: the decrypt under test undoes it
        dec = orc.limbs_to_ints(orc.decrypt(KEY, IT, add, minus, 1, b, ct))
        floats = np.concatenate([R.ref_unquantize(R.ref_unbatch(dec[es:es + ne], b, fb)[:sz], a, ebits, C)
                                 for es, ne, sz, a in zip(_starts(elems), elems, sizes, ALPHAS)])
        n_values = sum(sizes)
        out = eng.alloc(8 * (n_values + 1))
        eng.memset_dev(out, 0xFF, out.nbytes)
        din = eng.upload(W.int_limbs(W.wire_int(orc.limbs_to_ints(ct), b), W.n_limbs_of(n, b)))
        assert eng.unpack_decrypt_unbatch_unquantize_model_dev(IT, add, minus, [(sz, None, a, False) for sz, a in zip(sizes, ALPHAS)], ebits, fb, C, din, n, out)
        res = out.download(np.uint64, n_values + 1)
        assert int(res[n_values]) == GUARD, ("guard value", b, fb, flags, n)
        assert res[:n_values].tobytes() == floats.tobytes(), (b, fb, flags, n, np.flatnonzero(res[:n_values] != floats.view(np.uint64))[:4])


@pytest.mark.parametrize("case", ["int_bits=64", "n_add=2"])
def test_what_is_not_admitted_is_declined_with_the_output_untouched(engines, case):
    from flashe_amd.engine import SCHEME_DOUBLE
    b = 64 if case == "int_bits=64" else 120
    eng, n, fb = engines[b], 100, 20
    bs = b // fb
    x, u = eng.upload(np.zeros(n * bs, np.float32)), eng.upload(np.zeros(n * bs))
    packed, out = eng.alloc(8 * W.n_limbs_of(n, b)), eng.alloc(8 * n * bs)
    for buf in (packed, out):
        eng.memset_dev(buf, 0xFF, buf.nbytes)
    add = [5, 9] if case == "n_add=2" else [5]
    assert not eng.unpack_decrypt_unbatch_unquantize_model_dev(IT, add, [4], [(n * bs, None, 1.0, False)], 16, fb, C, packed, n, out)
    if case != "n_add=2":
        assert not eng.quantize_batch_encrypt_pack_model_dev(IT, IDX, SCHEME_DOUBLE, [(n * bs, x.ptr, 1.0, False)], 16, fb, u, n, packed)
    for buf in (packed, out):
        assert (buf.download(np.uint8, buf.nbytes) == 0xFF).all(), case
