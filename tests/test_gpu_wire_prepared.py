"""GPU: a precompute job's online client step straight to and from the packed wire form at int_bits 16 .. 64
(flashe_quantize_encrypt_prepared_pack_tensors_dev, flashe_unpack_decrypt_prepared_unquantize_model_dev; wire_prepared.hip), bit for bit.

No kernel of the engine goes into an expected value.  Way out, after prepare_encrypt(IT, IDX): the Python int wire_ref.expected builds from
the oracle's encrypt at (IT, IDX) of codec_ref's plaintexts.  Way back, after prepare_decrypt(IT, C): float64 BYTES against codec_ref's
unquantise of the oracle's decrypt with add [C], minus [0] of a wire integer of random elements.  Every output is pre-filled with 0xFF --
the kernels write every limb without a clear in front -- and a guard limb / value lies behind it.  Lengths around the tile of 64 T elements
counted from the END of the vector; wire_ref.three_layer_model: a tile straddles a row, float64 and float32 rows."""
import numpy as np
import pytest

import wire_ref as W
from wire_ref import C, EBITS, GUARD, IDX, IT, KEY

pytestmark = pytest.mark.gpu

WIDTHS = (16, 20, 23, 32, 33, 43, 64)
T = 4                                            # wire_prepared.hip, kPrepT: 64-element groups per tile
LENGTHS = (1, 5, 64 * T - 1, 64 * T, 64 * T + 1, 2 * 16 * 64 * T + 3)    # the last: more than one workgroup, a partial top limb


@pytest.fixture(scope="module")
def orc():
    from oracle import flashe_oracle
    return flashe_oracle


@pytest.fixture(scope="module")
def engines():
    from flashe_amd.engine import Engine
    return {b: Engine(KEY, b, device=0) for b in WIDTHS + (15, 65)}


def _way_out(eng, orc, b, scheme, n_jobs, n):
    from flashe_amd.engine import SCHEME_DOUBLE, SCHEME_SINGLE
    model, n_limbs = W.three_layer_model(n), W.n_limbs_of(n, b)
    want = W.expected(orc, model, b, scheme, n_jobs)[0]
    eng.prepare_encrypt(IT, IDX, SCHEME_DOUBLE if scheme == "double" else SCHEME_SINGLE, n, n_jobs)
    bufs = [eng.upload(x) if len(x) else None for x in model.held]
    rows = [(s, buf.ptr if buf else None, a, sh, code, fl)
            for s, buf, a, sh, code, fl in zip(model.starts, bufs, model.alphas, model.shifts, model.codes, model.flags)]
    packed = eng.alloc(8 * (n_limbs + 1))
    eng.memset_dev(packed, 0xFF, packed.nbytes)
    assert eng.quantize_encrypt_prepared_pack_tensors_dev(n, rows, EBITS, eng.upload(model.u), packed)
    got = packed.download(np.uint64, n_limbs + 1)
    assert int(got[n_limbs]) == GUARD, ("guard limb", b, scheme, n_jobs, n)
    assert int.from_bytes(got[:n_limbs].tobytes(), "little") == want, (b, scheme, n_jobs, n, np.flatnonzero(got[:n_limbs] != W.int_limbs(want, n_limbs))[:4])
    assert not eng.prepared_query(eng.PREPARED_ENCRYPT)[0], "consumed"


def _way_back(eng, orc, b, n_jobs, n):
    model, n_limbs = W.three_layer_model(n), W.n_limbs_of(n, b)
    halves = np.random.RandomState(b * 100003 + n).randint(0, 1 << 32, size=(n, 2)).astype(np.uint64)
    elems = [int(v) & ((1 << b) - 1) for v in (halves[:, 0] << np.uint64(32)) | halves[:, 1]]
    dec = orc.limbs_to_ints(orc.decrypt(KEY, IT, [C], [0], n_jobs, b, orc.ints_to_limbs(elems, b)))
    floats = W.row_floats(dec, model.starts, model.sizes, model.alphas)
    eng.prepare_decrypt(IT, C, n, n_jobs)
    out = eng.alloc(8 * (n + 1))
    eng.memset_dev(out, 0xFF, out.nbytes)
    din = eng.upload(W.int_limbs(W.wire_int(elems, b), n_limbs))
    back = [(int(s), None, a, False) for s, a in zip(model.starts, model.alphas)]
    assert eng.unpack_decrypt_prepared_unquantize_model_dev(IT, [], [], n, n_jobs, din, back, EBITS, C, out)
    res = out.download(np.uint64, n + 1)
    assert int(res[n]) == GUARD, ("guard value", b, n_jobs, n)
    assert res[:n].tobytes() == floats.tobytes(), (b, n_jobs, n, np.flatnonzero(res[:n] != floats.view(np.uint64))[:4])
    assert not eng.prepared_query(eng.PREPARED_DECRYPT)[0], "consumed"


@pytest.mark.parametrize("n_jobs", [1, 16])
@pytest.mark.parametrize("scheme", ["single", "double"])
@pytest.mark.parametrize("b", WIDTHS)
def test_way_out_matches_the_oracle_and_python_ints(engines, orc, b, scheme, n_jobs):
    for n in LENGTHS:
        _way_out(engines[b], orc, b, scheme, n_jobs, n)


@pytest.mark.parametrize("n_jobs", [1, 16])
@pytest.mark.parametrize("b", WIDTHS)
def test_way_back_matches_the_oracle_as_float64_bytes(engines, orc, b, n_jobs):
    for n in LENGTHS:
        _way_back(engines[b], orc, b, n_jobs, n)


def test_a_wave_takes_a_second_trip_on_one_cu(engines, orc):
    eng = engines[20]
    eng.set_cu_limit(1)
    try:
        _way_out(eng, orc, 20, "double", 16, LENGTHS[-1])
        _way_back(eng, orc, 20, 16, LENGTHS[-1])
    finally:
        eng.set_cu_limit(0)


@pytest.mark.parametrize("case", ["int_bits=15", "int_bits=65", "one extra prefix"])
def test_a_declined_call_leaves_the_outputs_and_the_cache(engines, case):
    from flashe_amd._lib import TENSOR_F32
    from flashe_amd.engine import SCHEME_DOUBLE
    b = {"int_bits=15": 15, "int_bits=65": 65}.get(case, 20)
    eng, n = engines[b], 100
    x, u = eng.upload(np.zeros(n, np.float32)), eng.upload(np.zeros(n))
    packed, out = eng.alloc(8 * W.n_limbs_of(n, b)), eng.alloc(8 * n)
    for buf in (packed, out):
        eng.memset_dev(buf, 0xFF, buf.nbytes)
    eng.prepare_encrypt(IT, IDX, SCHEME_DOUBLE, n, 1)
    eng.prepare_decrypt(IT, C, n, 1)
    try:
        assert not eng.unpack_decrypt_prepared_unquantize_model_dev(IT, [5] if case == "one extra prefix" else [], [], n, 1, packed, [(0, None, 1.0, False)], EBITS, C, out)
        if case != "one extra prefix":
            assert not eng.quantize_encrypt_prepared_pack_tensors_dev(n, [(0, x.ptr, 1.0, 0.0, TENSOR_F32, 0)], EBITS, u, packed)
        for buf in (packed, out):
            assert (buf.download(np.uint8, buf.nbytes) == 0xFF).all(), case
        assert eng.prepared_query(eng.PREPARED_ENCRYPT)[0] and eng.prepared_query(eng.PREPARED_DECRYPT)[0], case
    finally:
        eng.prepared_discard(eng.PREPARED_ENCRYPT | eng.PREPARED_DECRYPT)


def test_a_length_mismatch_raises_and_keeps_the_cache(engines):
    from flashe_amd._lib import TENSOR_F32
    from flashe_amd.engine import SCHEME_DOUBLE, FlasheError
    eng, n = engines[20], 100
    x, u, packed, out = eng.upload(np.zeros(n, np.float32)), eng.upload(np.zeros(n)), eng.alloc(8 * W.n_limbs_of(n, 20)), eng.alloc(8 * n)
    eng.prepare_encrypt(IT, IDX, SCHEME_DOUBLE, n, 1)
    eng.prepare_decrypt(IT, C, n, 1)
    try:
        with pytest.raises(FlasheError):
            eng.quantize_encrypt_prepared_pack_tensors_dev(n - 1, [(0, x.ptr, 1.0, 0.0, TENSOR_F32, 0)], EBITS, u, packed)
        with pytest.raises(FlasheError):
            eng.unpack_decrypt_prepared_unquantize_model_dev(IT, [], [], n - 1, 1, packed, [(0, None, 1.0, False)], EBITS, C, out)
        assert eng.prepared_query(eng.PREPARED_ENCRYPT)[:2] == (True, n) and eng.prepared_query(eng.PREPARED_DECRYPT)[:2] == (True, n)
    finally:
        eng.prepared_discard(eng.PREPARED_ENCRYPT | eng.PREPARED_DECRYPT)
