"""The int_bits = 128 specialisation of the summed double-mask chain (prf_dmask_sum128_kernel, prf_chain_sum128_tile.inc): one-limb
plaintexts, every ciphertext present.  Its whole tiles take a telescoped sum (sum of the plaintexts - D), buffer addressing and range
predicates in the chain's first and last tile only, so the shapes here aim at those edges: ragged ends, n not a multiple of 256, a
range that starts mid-tile, C = 1, 2 and 10, n_jobs 1 and 16.  Every ciphertext, the sum and the decrypt through D are compared with
the CPU oracle, into buffers poisoned first.

The summed launch only runs when the vector gives every wave of the chip two whole tiles (launch_prf_batch_sum), so the vectors
here are a few million elements long."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
KEY = bytes(range(32))
B = 128


@pytest.fixture(scope="module")
def E():
    from flashe_amd import engine
    return engine


def _pts(n, C, seed):
    return [np.random.Generator(np.random.PCG64(seed + c)).integers(0, 2 ** 64, n, dtype=np.uint64) for c in range(C)]


def _check(eng, oracle, it, idx, J, pts, dct, dsum, n, first, count):
    want_ct = [oracle.encrypt(KEY, it, c, "double", J, B, p)[first:first + count] for c, p in zip(idx, pts)]
    for c, d in zip(idx, dct):
        got = d.download(np.uint64, 2 * n).reshape(n, 2)[first:first + count]
        assert np.array_equal(got, want_ct[idx.index(c)]), ("ciphertext", c)
    hsum = dsum.download(np.uint64, 2 * n).reshape(n, 2)
    assert np.array_equal(hsum[first:first + count], oracle.aggregate_elem(want_ct, B)), "sum"
    # the decrypt with the chain's own (add, minus) runs as a combine with the D the launch wrote
    dout = eng.alloc_vec(n)
    eng.memset_dev(dout, 0x3C, dout.nbytes)
    eng.decrypt_range_dev(it, [idx[-1] + 1], [idx[0]], n, J, first, count, dsum.ptr + 16 * first, dout.ptr + 16 * first)
    got = dout.download(np.uint64, 2 * n).reshape(n, 2)[first:first + count]
    assert np.array_equal(got, oracle.decrypt(KEY, it, [idx[-1] + 1], [idx[0]], J, B, hsum)[first:first + count]), "decrypt"
    lo = sum(p[first:first + count].astype(object) for p in pts)
    assert [int(got[k, 0]) | (int(got[k, 1]) << 64) for k in (0, count // 2, count - 1)] == [int(lo[k]) for k in (0, count // 2, count - 1)]


@pytest.mark.parametrize("C", [1, 2, 10])
@pytest.mark.parametrize("J", [1, 16])
@pytest.mark.parametrize("n", [2_621_440, 2_600_037])          # whole tiles; ragged last tile (n not a multiple of 256)
def test_summed_chain_matches_oracle(E, oracle, C, J, n):
    eng = E.Engine(KEY, B, device=0)
    it, idx = 5, list(range(3, 3 + C))
    pts = _pts(n, C, 700 + C)
    dpt = [eng.upload(p) for p in pts]
    dct = [eng.alloc_vec(n) for _ in idx]
    for d in dct:
        eng.memset_dev(d, 0x5A, d.nbytes)
    dsum = eng.alloc_vec(n)
    eng.memset_dev(dsum, 0xA5, dsum.nbytes)
    eng.encrypt_batch_sum_dev(it, idx, E.SCHEME_DOUBLE, n, J, dpt, 1, dct, dsum)
    _check(eng, oracle, it, idx, J, pts, dct, dsum, n, 0, n)


@pytest.mark.parametrize("F, CNT", [(300_001, 2_400_000), (77, 2_200_117)])    # a range that starts (and ends) mid-tile
def test_range_starting_mid_tile(E, oracle, F, CNT):
    eng = E.Engine(KEY, B, device=0)
    n, it, idx, J = F + CNT + 1000, 9, [0, 1, 2, 3, 4], 16
    pts = _pts(n, len(idx), 900)
    dpt = [eng.upload(p) for p in pts]
    dct = [eng.alloc_vec(n) for _ in idx]
    for d in dct:
        eng.memset_dev(d, 0x5A, d.nbytes)
    dsum = eng.alloc_vec(n)
    eng.memset_dev(dsum, 0xA5, dsum.nbytes)
    eng.encrypt_batch_range_dev(it, idx, E.SCHEME_DOUBLE, n, J, F, CNT, [d.ptr + 8 * F for d in dpt], 1,
                                [d.ptr + 16 * F for d in dct], dsum.ptr + 16 * F)
    _check(eng, oracle, it, idx, J, pts, dct, dsum, n, F, CNT)
    # nothing outside the range was written
    for d in dct + [dsum]:
        raw = d.download(np.uint8, 16 * n)
        assert (raw[:16 * F] == (0x5A if d is not dsum else 0xA5)).all() and (raw[16 * (F + CNT):] == raw[0]).all()
