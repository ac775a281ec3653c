"""CPU test of the cohort client step's host-side front end (flashe_amd/block.py): the client-major draws where a stretch is longer than one
device call takes (_RNG_RUN_MAX, never crossed by the other tests: 2^26 draws), and the tensor-layer flags over every (host dtype, normalize,
wide / narrow arithmetic) combination.  On an engine double whose buffers record their uploads; touches no device."""
import itertools

import numpy as np
import pytest

from flashe_amd import _lib, block
from flashe_amd.quantize import _loop_dtype

RUN_MAX = 5


class _Buf:
    def __init__(self, nbytes):
        self.nbytes, self.ptr, self.uploads = int(nbytes), 1 << 20, []

    def upload_at(self, off, arr):
        arr = np.asarray(arr)
        assert arr.dtype == np.float64 and off + arr.nbytes <= self.nbytes
        self.uploads.append((int(off), arr.copy()))
        return self


class _Engine:
    def __init__(self):
        self.bufs = []

    def alloc(self, nbytes):
        self.bufs.append(_Buf(nbytes))
        return self.bufs[-1]

    def numpy_random_dev(self, *a, **kw):
        raise AssertionError("FLASHE_DEVICE_RNG=0: the draws come from the host")


def _state():
    st = np.random.get_state()
    return st[0], st[1].tobytes(), st[2]


@pytest.fixture
def eng(monkeypatch):
    monkeypatch.setattr(block, "_RNG_RUN_MAX", RUN_MAX)
    monkeypatch.setenv("FLASHE_DEVICE_RNG", "0")
    return _Engine()


def _tiles(uploads, first, count):
    """The uploads cover draws [first, first + count) exactly once, in ascending order, in chunks of at most RUN_MAX draws."""
    at = 8 * first
    for off, vals in uploads:
        assert off == at and 1 <= vals.size <= RUN_MAX
        at += vals.nbytes
    assert at == 8 * (first + count)


def test_global_stream_draws_are_one_stretch_cut_at_the_run_length(eng):
    C, per = 3, 7
    np.random.seed(41)
    du = block._cohort_draws(eng, C, per, None)
    after = _state()
    assert eng.bufs == [du] and du.nbytes == 8 * C * per
    _tiles(du.uploads, 0, C * per)
    np.random.seed(41)
    assert np.array_equal(np.concatenate([v for _o, v in du.uploads]), np.random.random(C * per))
    assert _state() == after


def test_seeded_draws_start_at_each_clients_seed_and_no_chunk_spans_two_clients(eng):
    C, per, seeds = 3, 7, [5, 6, 7]
    np.random.seed(41)
    du = block._cohort_draws(eng, C, per, seeds)
    after = _state()
    assert du.nbytes == 8 * C * per
    for c, seed in enumerate(seeds):
        mine = [(off, v) for off, v in du.uploads if 8 * per * c <= off < 8 * per * (c + 1)]
        _tiles(mine, per * c, per)                                  # (a chunk that ran into the next client would end past its stretch)
        np.random.seed(seed)
        assert np.array_equal(np.concatenate([v for _o, v in mine]), np.random.random(per))
    assert sum(v.size for _o, v in du.uploads) == C * per
    assert [off for off, _v in du.uploads] == sorted(off for off, _v in du.uploads)
    np.random.seed(seeds[-1])
    np.random.random(per)
    assert _state() == after


@pytest.mark.parametrize("seeds", [None, [9]])
def test_no_draws_no_upload(eng, seeds):
    np.random.seed(41)
    before = _state()
    if seeds is not None:
        np.random.seed(seeds[0])                                     # (a seeded client re-seeds, and draws nothing)
        before = _state()
        np.random.seed(41)
    du = block._cohort_draws(eng, 1, 0, seeds)
    assert du.nbytes == 16 and du.uploads == [] and _state() == before


# alphas / means that make NumPy compute `float32 array <op> scalar` in float64 (a NumPy scalar of that type), and ones that do not
SCALARS = [np.float64(0.25), 0.25, np.float32(0.25)]


@pytest.mark.parametrize("hdt, normalize, alpha, mean",
                         list(itertools.product([np.dtype(np.float32), np.dtype(np.float64)], [False, True], SCALARS, SCALARS)))
def test_tensor_flags_follow_numpys_loop_dtype(hdt, normalize, alpha, mean):
    shift, flags = block._tensor_flags(hdt, alpha, normalize, mean)
    want = 0
    if hdt != np.float64 and _loop_dtype(hdt, alpha) == np.float64:
        want |= _lib.TENSOR_LOOP_F64
    if normalize:
        want |= _lib.TENSOR_SHIFT
        if hdt == np.float32 and _loop_dtype(hdt, -mean) == np.float64:
            want |= _lib.TENSOR_SHIFT_WIDE
    assert flags == want
    assert isinstance(shift, float) and shift == (-0.25 if normalize else 0.0)
    assert not flags & ~(_lib.TENSOR_LOOP_F64 | _lib.TENSOR_SHIFT | _lib.TENSOR_SHIFT_WIDE)
    if hdt == np.float64:
        assert flags == (_lib.TENSOR_SHIFT if normalize else 0)      # a float64 layer is never widened


def test_the_scalars_exercise_both_answers_of_loop_dtype():
    answers = {_loop_dtype(np.float32, s) for s in SCALARS}
    assert answers == {np.dtype(np.float32), np.dtype(np.float64)}
