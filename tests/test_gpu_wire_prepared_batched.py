"""GPU: a BATCHED precompute job's online client step straight to and from the packed wire form at int_bits 65 .. 128
(flashe_quantize_batch_encrypt_prepared_pack_model_dev, flashe_unpack_decrypt_prepared_unbatch_unquantize_model_dev; wire_prepared.hip), bit
for bit.  Way out, after prepare_encrypt(IT, IDX): codec_ref.ref_quantize and ref_batch per row -> the oracle's encrypt -> wire_ref.wire_int,
compared as a Python int.  Way back, after prepare_decrypt(IT, C): float64 BYTES against ref_unquantize(ref_unbatch(the oracle's decrypt with
add [C], minus [0])).  Outputs pre-filled with 0xFF, a guard behind each.  Three rows; the second one's padded last element lies inside a tile."""
import functools

import numpy as np
import pytest

import codec_ref as R
import wire_ref as W
from wire_ref import C, GUARD, IDX, IT, KEY

pytestmark = pytest.mark.gpu

WIDTHS = ((65, 20), (120, 20), (127, 20), (120, 17), (128, 21))      # bs 3 (the generic walk), 6, 6 (spare top bits), 7, 6
N_ELEMS = (1, 63, 64, 65, 2 * 16 * 64 + 3)
ALPHAS = (8.17121, 3e-3, 6.5)


@functools.lru_cache(maxsize=None)
def _model(bs, n_elems):
    """(arrays, sizes in values, sizes in elements, draws): a float64 row of two elements, the last one padded; a float32 row whose padded
    last element lies mid-vector; a float32 row of whole elements.  n_elems = 1: one value alone."""
    if n_elems == 1:
        rows = [(np.float32, 1, 1)]
    else:
        e1 = (n_elems - 2) // 2
        rows = [(np.float64, bs + 2, 2), (np.float32, e1 * bs - 1, e1), (np.float32, (n_elems - 2 - e1) * bs, n_elems - 2 - e1)]
    xs = [R.layer_fill(dt, ALPHAS[l], s, seed=l) for l, (dt, s, _e) in enumerate(rows)]
    sizes, elems = [s for _dt, s, _e in rows], [e for _dt, _s, e in rows]
    assert [(s + bs - 1) // bs for s in sizes] == elems and sum(elems) == n_elems
    return xs, sizes, elems, R.mixed_draws(sum(sizes))


def _starts(v):
    return [int(s) for s in np.concatenate([[0], np.cumsum(v)[:-1]])]


@pytest.fixture(scope="module")
def orc():
    from oracle import flashe_oracle
    return flashe_oracle


@pytest.fixture(scope="module")
def engines():
    from flashe_amd.engine import Engine
    return {b: Engine(KEY, b, device=0) for b in sorted({b for b, _f in WIDTHS})}


@pytest.mark.parametrize("scheme", ["single", "double"])
@pytest.mark.parametrize("b,fb", WIDTHS)
def test_way_out_matches_the_oracle_and_python_ints(engines, orc, b, fb, scheme):
    from flashe_amd.engine import SCHEME_DOUBLE, SCHEME_SINGLE
    eng, bs, ebits = engines[b], b // fb, fb - 2
    for n in N_ELEMS:
        xs, sizes, _elems, u = _model(bs, n)
        pt = [t % (1 << b) for x, a, s, sz in zip(xs, ALPHAS, _starts(sizes), sizes) for t in R.ref_batch(R.ref_quantize(x, a, ebits, u[s:s + sz]), b, fb)]
        want = W.wire_int(orc.limbs_to_ints(orc.encrypt(KEY, IT, IDX, scheme, 1, b, orc.ints_to_limbs(pt, b))), b)
        eng.prepare_encrypt(IT, IDX, SCHEME_DOUBLE if scheme == "double" else SCHEME_SINGLE, n, 1)
        bufs = [eng.upload(x) for x in xs]
        rows = [(sz, buf.ptr, a, x.dtype == np.float64) for sz, buf, a, x in zip(sizes, bufs, ALPHAS, xs)]
        n_limbs = W.n_limbs_of(n, b)
        packed = eng.alloc(8 * (n_limbs + 1))
        eng.memset_dev(packed, 0xFF, packed.nbytes)
        assert eng.quantize_batch_encrypt_prepared_pack_model_dev(rows, ebits, fb, eng.upload(u), n, packed)
        got = packed.download(np.uint64, n_limbs + 1)
        assert int(got[n_limbs]) == GUARD, ("guard limb", b, fb, scheme, n)
        assert int.from_bytes(got[:n_limbs].tobytes(), "little") == want, (b, fb, scheme, n, np.flatnonzero(got[:n_limbs] != W.int_limbs(want, n_limbs))[:4])
        assert not eng.prepared_query(eng.PREPARED_ENCRYPT)[0], "consumed"


@pytest.mark.parametrize("b,fb", WIDTHS)
def test_way_back_matches_the_oracle_as_float64_bytes(engines, orc, b, fb):
    eng, bs, ebits = engines[b], b // fb, fb - 2
    plane = R.sum_plane(ebits, C, int_bits=fb, n_random=500)
    for n in N_ELEMS:
        _xs, sizes, elems, _u = _model(bs, n)
        vals = [[plane[(s + j) % len(plane)] for j in range(sz)] for s, sz in zip(_starts(sizes), sizes)]
        pt = [t % (1 << b) for v in vals for t in R.ref_batch(v, b, fb)]
        ct = orc.decrypt(KEY, IT, [0], [C], 1, b, orc.ints_to_limbs(pt, b))                     # the inverse mask: the decrypt under test undoes it
        dec = orc.limbs_to_ints(orc.decrypt(KEY, IT, [C], [0], 1, b, ct))
        floats = np.concatenate([R.ref_unquantize(R.ref_unbatch(dec[es:es + ne], b, fb)[:sz], a, ebits, C)
                                 for es, ne, sz, a in zip(_starts(elems), elems, sizes, ALPHAS)])
        n_values = sum(sizes)
        eng.prepare_decrypt(IT, C, n, 1)
        out = eng.alloc(8 * (n_values + 1))
        eng.memset_dev(out, 0xFF, out.nbytes)
        din = eng.upload(W.int_limbs(W.wire_int(orc.limbs_to_ints(ct), b), W.n_limbs_of(n, b)))
        assert eng.unpack_decrypt_prepared_unbatch_unquantize_model_dev(IT, [], [], 1, [(sz, None, a, False) for sz, a in zip(sizes, ALPHAS)], ebits, fb, C, din, n, out)
        res = out.download(np.uint64, n_values + 1)
        assert int(res[n_values]) == GUARD, ("guard value", b, fb, n)
        assert res[:n_values].tobytes() == floats.tobytes(), (b, fb, n, np.flatnonzero(res[:n_values] != floats.view(np.uint64))[:4])
        assert not eng.prepared_query(eng.PREPARED_DECRYPT)[0], "consumed"
