"""GPU: the dense client step straight to and from the packed wire form (flashe_quantize_encrypt_pack_tensors_dev,
flashe_unpack_decrypt_unquantize_model_dev; wire.hip) through the C ABI wrappers, bit for bit.

Way out: the expected limbs are the Python int sum(ct[j] << (b * (n - 1 - j))) (jzf_weights.py `_to_bytes_old`), ct = the oracle's encrypt of
the plaintexts tests/codec_ref.py quantises -- deliberately no other kernel of this engine.  Way back: float64 BYTES against codec_ref's
unquantise of the oracle's decrypt of the same elements.  Lengths: the smallest at which each piece can go wrong -- n = 1, n = 5 < n_jobs,
one tile either side of its edge (64 m - 1, 64 m -- where n b % 64 == 0 --, 64 m + 1) and 2 * 16 * 64 m + 3: more than one workgroup, shared
limbs across workgroups, a partial top limb.  Three layers (float64 of 7 values, two float32, different alphas): a block straddles a row."""
import numpy as np
import pytest

import wire_ref as W
from wire_ref import C, EBITS, IDX, IT, KEY

pytestmark = pytest.mark.gpu

WIDTHS = (16, 20, 23, 32, 33, 43, 64)           # m = 8, 6, 5, 4, 3, 2, 2: field widths 128, 120, 115, 128, 99, 86, 128


def _lengths(b):
    m = 128 // b
    return (1, 5, 64 * m - 1, 64 * m, 64 * m + 1, 2 * 16 * 64 * m + 3)


def _round_trip(eng, orc, b, scheme, n_jobs, n):
    W.round_trip(eng, orc, b, scheme, n_jobs, W.three_layer_model(n))


@pytest.fixture(scope="module")
def orc():
    from oracle import flashe_oracle
    return flashe_oracle


@pytest.fixture(scope="module")
def engines():
    from flashe_amd.engine import Engine
    return {b: Engine(KEY, b, device=0) for b in WIDTHS + (15, 65)}


@pytest.mark.parametrize("n_jobs", [1, 16])
@pytest.mark.parametrize("scheme", ["single", "double"])
@pytest.mark.parametrize("b", WIDTHS)
def test_both_directions_match_the_oracle_and_python_ints(engines, orc, b, scheme, n_jobs):
    for n in _lengths(b):
        _round_trip(engines[b], orc, b, scheme, n_jobs, n)


def test_a_wave_takes_a_second_trip_on_one_cu(engines, orc):
    eng = engines[20]
    eng.set_cu_limit(1)
    try:
        _round_trip(eng, orc, 20, "double", 16, _lengths(20)[-1])
    finally:
        eng.set_cu_limit(0)


@pytest.mark.parametrize("case", ["n_add=2", "int_bits=15", "int_bits=65"])
def test_what_is_not_admitted_is_declined_with_the_output_untouched(engines, case):
    from flashe_amd._lib import TENSOR_F32
    from flashe_amd.engine import SCHEME_DOUBLE
    b = {"int_bits=15": 15, "int_bits=65": 65}.get(case, 20)
    eng, n = engines[b], 100
    n_limbs = (n * b + 63) // 64
    x, u = eng.upload(np.zeros(n, np.float32)), eng.upload(np.zeros(n))
    packed, out = eng.alloc(8 * n_limbs), eng.alloc(8 * n)
    for buf in (packed, out):
        eng.memset_dev(buf, 0xFF, buf.nbytes)
    add = [5, 9] if case == "n_add=2" else [5]
    assert not eng.unpack_decrypt_unquantize_model_dev(IT, add, [4], n, 1, packed, [(0, None, 1.0, False)], EBITS, C, out)
    if case != "n_add=2":
        assert not eng.quantize_encrypt_pack_tensors_dev(IT, IDX, SCHEME_DOUBLE, n, 1, [(0, x.ptr, 1.0, 0.0, TENSOR_F32, 0)], EBITS, u, packed)
    for buf in (packed, out):
        assert (buf.download(np.uint8, buf.nbytes) == 0xFF).all(), case
