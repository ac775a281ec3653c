"""GPU: the dense client step straight to and from the packed wire form (flashe_quantize_encrypt_pack_tensors_dev,
flashe_unpack_decrypt_unquantize_model_dev; wire.hip) through the C ABI wrappers, bit for bit.

Way out: the expected limbs are the Python int sum(ct[j] << (b * (n - 1 - j))) (jzf_weights.py `_to_bytes_old`), ct = the oracle's encrypt of
the plaintexts tests/codec_ref.py quantises -- deliberately no other kernel of this engine.  Way back: float64 BYTES against codec_ref's
unquantise of the oracle's decrypt of the same elements.  Lengths: the smallest at which each piece can go wrong -- n = 1, n = 5 < n_jobs,
one tile either side of its edge (64 m - 1, 64 m -- where n b % 64 == 0 --, 64 m + 1) and 2 * 16 * 64 m + 3: more than one workgroup, shared
limbs across workgroups, a partial top limb.  Three layers (float64 of 7 values, two float32, different alphas): a block straddles a row."""
import numpy as np
import pytest

import codec_ref as R

pytestmark = pytest.mark.gpu

KEY = bytes(range(32))
IT, IDX, EBITS, C = 9, 4, 12, 3
ALPHAS = (8.17121, 3e-3, 6.5)
WIDTHS = (16, 20, 23, 32, 33, 43, 64)           # m = 8, 6, 5, 4, 3, 2, 2: field widths 128, 120, 115, 128, 99, 86, 128


def _lengths(b):
    m = 128 // b
    return (1, 5, 64 * m - 1, 64 * m, 64 * m + 1, 2 * 16 * 64 * m + 3)


def _wire_int(ct, b):
    """sum(ct[j] << (b * (n - 1 - j))), 256 elements at a time (the one-by-one sum is quadratic in n)."""
    acc = 0
    for at in range(0, len(ct), 256):
        part = 0
        for v in ct[at:at + 256]:
            part = (part << b) | int(v)
        acc = (acc << (b * len(ct[at:at + 256]))) | part
    return acc


def _model(n):
    """(sizes, dtypes, arrays, draws) of the three-layer model of n values."""
    s0 = min(7, max(1, n // 2))
    s1 = (n - s0) // 2
    sizes, dts = (s0, s1, n - s0 - s1), (np.float64, np.float32, np.float32)
    xs = [R.layer_fill(dt, a, s, seed=l) if s else np.zeros(0, dt) for l, (dt, a, s) in enumerate(zip(dts, ALPHAS, sizes))]
    return sizes, dts, xs, R.mixed_draws(n)


def _expected(orc, b, scheme, n_jobs, n):
    sizes, dts, xs, u = _model(n)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(int)
    q = np.concatenate([R.ref_quantize(x, a, EBITS, u[s:s + len(x)]) for x, a, s in zip(xs, ALPHAS, starts) if len(x)])
    pt = (q.astype(np.uint64) & np.uint64((1 << b) - 1))
    ct = orc.limbs_to_ints(orc.encrypt(KEY, IT, IDX, scheme, n_jobs, b, pt))
    add, minus = ([IDX + 1], [IDX]) if scheme == "double" else ([], [IDX])          # what undoes one client's own mask
    dec = orc.limbs_to_ints(orc.decrypt(KEY, IT, add, minus, n_jobs, b, orc.ints_to_limbs(ct, b)))
    floats = np.concatenate([R.ref_unquantize(dec[s:s + sz], a, EBITS, C) for s, sz, a in zip(starts, sizes, ALPHAS) if sz])
    return sizes, starts, dts, xs, u, _wire_int(ct, b), add, minus, floats


def _round_trip(eng, orc, b, scheme, n_jobs, n):
    from flashe_amd._lib import TENSOR_F32, TENSOR_F64
    from flashe_amd.engine import SCHEME_DOUBLE, SCHEME_SINGLE
    sizes, starts, dts, xs, u, want, add, minus, floats = _expected(orc, b, scheme, n_jobs, n)
    n_limbs = (n * b + 63) // 64
    bufs = [eng.upload(x) if len(x) else None for x in xs]
    rows = [(int(s), buf.ptr if buf else None, a, 0.0, TENSOR_F64 if dt == np.float64 else TENSOR_F32, 0) for s, buf, a, dt in zip(starts, bufs, ALPHAS, dts)]
    packed = eng.alloc(8 * (n_limbs + 1))
    eng.memset_dev(packed, 0xFF, packed.nbytes)
    assert eng.quantize_encrypt_pack_tensors_dev(IT, IDX, SCHEME_DOUBLE if scheme == "double" else SCHEME_SINGLE, n, n_jobs, rows, EBITS, eng.upload(u), packed)
    got = packed.download(np.uint64, n_limbs + 1)
    assert int(got[n_limbs]) == (1 << 64) - 1, ("guard limb", b, scheme, n_jobs, n)
    assert int.from_bytes(got[:n_limbs].tobytes(), "little") == want, ("way out", b, scheme, n_jobs, n)
    # way back: the expected integer itself goes in
    out = eng.alloc(8 * (n + 1))
    eng.memset_dev(out, 0xFF, out.nbytes)
    din = eng.upload(np.frombuffer(want.to_bytes(8 * n_limbs, "little"), dtype=np.uint64))
    back = [(int(s), None, a, False) for s, a in zip(starts, ALPHAS)]
    assert eng.unpack_decrypt_unquantize_model_dev(IT, add, minus, n, n_jobs, din, back, EBITS, C, out)
    res = out.download(np.uint64, n + 1)
    assert int(res[n]) == (1 << 64) - 1, ("guard value", b, scheme, n_jobs, n)
    assert res[:n].tobytes() == floats.tobytes(), ("way back", b, scheme, n_jobs, n, np.flatnonzero(res[:n] != floats.view(np.uint64))[:4])


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
