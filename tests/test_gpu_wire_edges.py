"""GPU: the packed wire kernels (prf_small_pack_kernel / prf_small_unpack_kernel, wire.hip) where tests/test_gpu_wire_client_step.py does
not reach, through the same two entry points and against the same references (tests/wire_ref.py: Python ints, the CPU oracle's cipher,
codec_ref's codec -- no other kernel of this engine), bit for bit:

  A  every admitted width 16 .. 64 (m = 128 // b = 2 .. 8, every field width m b), a tile either side of its edge and several tiles;
  B  float64 rows long enough that whole tiles lie inside them (the 16-byte run loads of a float64 row, at even and at odd element
     offsets), with row boundaries that cut tiles;
  C  staged rows (float16, bfloat16, SHIFT, SHIFT_WIDE, LOOP_F64 -- a float32 row computed in float64 --, a shifted float64 row), read
     by whole tiles from the staged copy;
  D  the way back over sums with high bits set: the ends of a real sum's range, 2^b - 1, 2^(b-1), and from 54 bits on values whose
     int -> float64 conversion has to round;
  E  the add-only prefix form ([a], []) of the way back;
  F  chunking edges: one element per chunk (every lane of every tile ragged), chunks of two lengths whose ends fall in mid tile, chunks
     of whole blocks only on one compute unit.

With m = 128 // b a tile is T = 64 m elements.  wire_ref.tiles restates the tiling, and the tests assert on their inputs alone that the
shapes reach the paths they are there for.  Integers are compared exactly, floats as bytes: no tolerance anywhere."""
import contextlib
import functools

import numpy as np
import pytest

import codec_ref as R
import wire_ref as W
from wire_ref import C, EBITS, IT, KEY

pytestmark = pytest.mark.gpu

ALL_WIDTHS = tuple(range(16, 65))
B_ALPHAS = W.ALPHAS + (1.0,)
# storage, alpha, shift, wide, loop64 of the staged rows
STAGED = (("float16", 8.17121, None, False, False), ("bfloat16", 3e-3, None, False, False), ("float32", 6.5, 0.0625, False, False),
          ("float32", 1.0, 0.0625, True, False), ("float32", 0.1, None, False, True), ("float64", 8.17121, 0.0625, False, False))
BIG_EBITS = 53                                   # group D's extra case: the widest sum the 64-bit element holds at C = 3 is 3 (2^53 - 1)

# the reference is platform-defined where the largest scaled image overflows the dtype: no alpha used here does (asserted, not filtered)
for _alpha in set(B_ALPHAS) | {row[1] for row in STAGED}:
    for _dt in (np.float32, np.float64):
        assert not R.overflows(_dt, _alpha, EBITS), (_dt, _alpha)


def _T(b):
    return 64 * (128 // b)


@pytest.fixture(scope="module")
def orc():
    from oracle import flashe_oracle
    return flashe_oracle


@contextlib.contextmanager
def _engine(b):
    from flashe_amd.engine import Engine
    eng = Engine(KEY, b, device=0)
    try:
        yield eng
    finally:
        eng.close()


# ================================================================================================ A: every admitted width
def _sweep_lengths(b):
    T = _T(b)
    return (T - 1, T + 1, 3 * T + 5)


@pytest.mark.parametrize("b", ALL_WIDTHS)
def test_every_admitted_width_round_trips(orc, b):
    assert {128 // w for w in ALL_WIDTHS} == {2, 3, 4, 5, 6, 7, 8}
    met = {(n * w) % 64 for w in ALL_WIDTHS for n in _sweep_lengths(w)}
    assert 0 in met and any(v % 2 for v in met), sorted(met)
    with _engine(b) as eng:
        for scheme in ("single", "double"):
            for n_jobs in (1, 3):
                for n in _sweep_lengths(b):
                    W.round_trip(eng, orc, b, scheme, n_jobs, W.three_layer_model(n))


# ================================================================================================ B: long float64 rows
LONG_WIDTHS = (16, 17, 23, 32, 33, 64)


@functools.lru_cache(maxsize=None)
def _long_model(T):
    sizes = (2 * T + 3, T + 1, 3 * T - 2, 5)
    kinds = ("float64", "float32", "float64", "float32")
    return W.cohort_wire_model([(st, a, None, False, False, s) for st, a, s in zip(kinds, B_ALPHAS, sizes)], seed=T)


def _f64_row_offsets(model, n_jobs, m):
    """r = e0 - start of every whole tile inside a float64 row, and whether a tile is cut by a row boundary."""
    offs = []
    for s, size, code in zip(model.starts, model.sizes, model.codes):
        if code == R.F64:
            offs += [e0 - s for e0, _e1 in W.whole_tiles_in(model.n, n_jobs, m, s, s + size)]
    cut = any(not ragged and any(e0 < s < e1 for s in model.starts) for e0, e1, ragged in W.tiles(model.n, n_jobs, m))
    return offs, cut


def test_long_float64_rows_hold_whole_tiles_at_even_and_odd_offsets():
    """On the inputs alone: at every width and n_jobs whole tiles lie inside both float64 rows and a row boundary cuts a whole tile; over
    the sweep the lanes' first values lie at even and at odd elements of a float64 row (16-byte aligned and not)."""
    parities = set()
    for b in LONG_WIDTHS:
        m = 128 // b
        model = _long_model(_T(b))
        for n_jobs in (1, 16):
            offs, cut = _f64_row_offsets(model, n_jobs, m)
            assert len(offs) >= 2 and cut, (b, n_jobs, offs, cut)
            parities |= {(r + lane * m) % 2 for r in offs for lane in (0, 1)}
        for s, size, code in zip(model.starts, model.sizes, model.codes):
            if code == R.F64:
                assert W.whole_tiles_in(model.n, 1, m, s, s + size), (b, s)
    assert parities == {0, 1}


@pytest.mark.parametrize("n_jobs", [1, 16])
@pytest.mark.parametrize("scheme", ["single", "double"])
@pytest.mark.parametrize("b", LONG_WIDTHS)
def test_long_float64_rows_and_row_boundaries_inside_whole_tiles(orc, b, scheme, n_jobs):
    with _engine(b) as eng:
        W.round_trip(eng, orc, b, scheme, n_jobs, _long_model(_T(b)))


# ================================================================================================ C: staged rows
STAGED_WIDTHS = (16, 20, 43)
STAGED_JOBS = 16


@functools.lru_cache(maxsize=None)
def _staged_model(b):
    """Every row 2 T + 1 values -- a whole tile fits wherever the row begins -- and the last one as much longer as makes n a multiple of
    n_jobs m: every chunk is whole blocks, so every tile is read a row at a time or cut by a row boundary, none is ragged."""
    m, T = 128 // b, _T(b)
    size = 2 * T + 1
    pad = -(len(STAGED) * size) % (STAGED_JOBS * m)
    return W.cohort_wire_model([row + (size + (pad if li == len(STAGED) - 1 else 0),) for li, row in enumerate(STAGED)], seed=b)


@pytest.mark.parametrize("scheme", ["single", "double"])
@pytest.mark.parametrize("b", STAGED_WIDTHS)
def test_staged_rows_are_read_by_whole_tiles(orc, b, scheme):
    model, m = _staged_model(b), 128 // b
    assert model.codes == (R.F16, R.BF16, R.F32, R.F32, R.F32, R.F64)
    assert model.flags == (0, 0, R.SHIFT, R.SHIFT | R.SHIFT_WIDE, R.LOOP_F64, R.SHIFT)
    assert [x.dtype for x in model.ref] == [np.float32] * 4 + [np.float64] * 2            # LOOP_F64: a float64 row in the staged copy
    assert not any(ragged for _e0, _e1, ragged in W.tiles(model.n, STAGED_JOBS, m))
    for s, size in zip(model.starts, model.sizes):
        assert size >= _T(b) + 1 and W.whole_tiles_in(model.n, STAGED_JOBS, m, s, s + size), (b, s)
    with _engine(b) as eng:
        W.round_trip(eng, orc, b, scheme, STAGED_JOBS, model)


# ================================================================================================ D: large sums on the way back
SUM_WIDTHS = (16, 17, 32, 33, 53, 54, 63, 64)
SUM_ALPHAS = W.ALPHAS


def _sum_values(b, ebits, n):
    """2^b - 1, 2^(b-1), 2^(b-1) - 1 and codec_ref.sum_plane's aggregates below 2^b (the ends of the range a sum of C clients has, the
    places where int -> float64 rounds half to even, random values of every bit length), tiled to n."""
    pts = [(1 << b) - 1, 1 << (b - 1), (1 << (b - 1)) - 1] + [v % (1 << b) for v in R.sum_plane(ebits, C, int_bits=b, n_random=300)]
    return [pts[j % len(pts)] for j in range(n)]


def _sum_rows(b):
    """Three rows over n = 2 T + 7: tile 0 inside row 0, tile 1 cut by both boundaries, the tail inside row 2."""
    T = _T(b)
    return 2 * T + 7, (0, T + 5, 2 * T - 3), (T + 5, T - 8, 10)


def _check_large_sums(orc, b, ebits):
    n, starts, sizes = _sum_rows(b)
    vals = _sum_values(b, ebits, n)
    assert max(vals) == (1 << b) - 1 and (b < 54 or any(float(v) != v for v in vals[:64 * (128 // b)]))       # rounding, inside tile 0
    (t0, t1, *_rest) = W.tiles(n, 1, 128 // b)
    assert not t0[2] and t0[1] <= sizes[0] and not t1[2] and t1[0] < starts[1] < starts[2] < t1[1]
    floats = W.row_floats(vals, starts, sizes, SUM_ALPHAS, ebits, C)
    with _engine(b) as eng:
        for scheme in ("single", "double"):
            for n_jobs in (1, 16):
                ct = orc.limbs_to_ints(orc.encrypt(KEY, IT, W.IDX, scheme, n_jobs, b, np.array(vals, dtype=np.uint64)))
                add, minus = W.own_mask(scheme)
                assert orc.limbs_to_ints(orc.decrypt(KEY, IT, add, minus, n_jobs, b, orc.ints_to_limbs(ct, b))) == vals
                W.check_way_back(eng, W.wire_int(ct, b), n, b, add, minus, n_jobs, starts, SUM_ALPHAS, floats, (b, scheme, n_jobs, n, ebits),
                                 ebits=ebits, num_clients=C)


@pytest.mark.parametrize("b", SUM_WIDTHS)
def test_large_sums_come_back_as_the_reference_floats(orc, b):
    _check_large_sums(orc, b, EBITS)


def test_large_sums_of_53_bit_values_at_64_bits(orc):
    """element_bits = 53, C = 3 at int_bits 64: the back end admits element_bits up to 62, so 53 is taken as it is -- the denominator
    3 (2^53 - 1) is itself no float64, and every sum near the top of the range is rounded on its way to one."""
    _check_large_sums(orc, 64, BIG_EBITS)


# ================================================================================================ E: the add-only prefix form
@pytest.mark.parametrize("n_jobs", [1, 16])
@pytest.mark.parametrize("b", [16, 23, 64])
def test_the_add_only_prefix_form(orc, b, n_jobs):
    a = W.IDX + 3
    with _engine(b) as eng:
        for n in (5, _T(b) + 1):
            model = W.three_layer_model(n)
            rng = np.random.Generator(np.random.PCG64(1000 * b + n))
            elems = rng.integers(0, 1 << b, n, dtype=np.uint64, endpoint=False) if b < 64 else rng.integers(0, (1 << 64) - 1, n, dtype=np.uint64, endpoint=True)
            dec = orc.limbs_to_ints(orc.decrypt(KEY, IT, [a], [], n_jobs, b, elems))
            floats = W.row_floats(dec, model.starts, model.sizes, model.alphas)
            W.check_way_back(eng, W.wire_int([int(v) for v in elems], b), n, b, [a], [], n_jobs, model.starts, model.alphas, floats, (b, "add-only", n_jobs, n))


# ================================================================================================ F: chunking edges
CHUNK_WIDTHS = (16, 20, 43)


@pytest.mark.parametrize("scheme", ["single", "double"])
@pytest.mark.parametrize("b", CHUNK_WIDTHS)
def test_one_element_per_chunk_makes_every_lane_ragged(orc, b, scheme):
    n = 3 * 64 + 1
    tl = W.tiles(n, n, 128 // b)
    assert len(tl) == 4 and all(ragged for _e0, _e1, ragged in tl) and [e1 - e0 for e0, e1, _r in tl] == [64, 64, 64, 1]
    with _engine(b) as eng:
        W.round_trip(eng, orc, b, scheme, n, W.three_layer_model(n))


@pytest.mark.parametrize("scheme", ["single", "double"])
@pytest.mark.parametrize("b", CHUNK_WIDTHS)
def test_chunks_of_two_lengths_end_in_mid_tile(orc, b, scheme):
    m, T = 128 // b, _T(b)
    n = 7 * (T // 2) + 3
    d, r = divmod(n, 7)
    assert r == 3 and -(-(d + 1) // m) != -(-d // m)                       # three longer chunks, of one block more
    ends = [c * (d + 1) for c in range(1, r + 1)] + [r * (d + 1) + c * d for c in range(1, 7 - r)]
    tl = W.tiles(n, 7, m)
    assert all(any(e0 < end < e1 for e0, e1, _r in tl) for end in ends), (ends, tl)
    with _engine(b) as eng:
        W.round_trip(eng, orc, b, scheme, 7, W.three_layer_model(n))


@pytest.mark.parametrize("scheme", ["single", "double"])
@pytest.mark.parametrize("b", CHUNK_WIDTHS)
def test_chunks_of_whole_blocks_on_one_compute_unit(orc, b, scheme):
    m, T = 128 // b, _T(b)
    n = 3 * T * m
    assert not any(ragged for _e0, _e1, ragged in W.tiles(n, 3, m))
    with _engine(b) as eng:
        eng.set_cu_limit(1)
        W.round_trip(eng, orc, b, scheme, 3, W.three_layer_model(n))


# ================================================================================================ the reference integer itself
@pytest.mark.parametrize("b", [16, 17, 43, 64])
def test_the_reference_integer_is_what_compress_builds(b):
    """wire_ref.wire_int against weights.to_big_int / TransferableWeights on host arrays (their packing runs on the device)."""
    from flashe_amd.weights import TransferableWeights, to_big_int
    rng = np.random.Generator(np.random.PCG64(b))
    for n in (1, 5, 129):
        vals = [int(v) for v in rng.integers(0, (1 << b) - 1, n, dtype=np.uint64, endpoint=True)]
        vals[-1] |= 1
        vals[0] = (1 << b) - 1
        arr = np.array(vals, dtype=object)
        assert to_big_int(arr, b) == (W.wire_int(vals, b), n)
        assert TransferableWeights({"w": arr}, b).unboxed["w"] == W.wire_int(vals, b)
