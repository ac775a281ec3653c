"""The chain decrypt mask (flashe_ctx::ChainDmask, abi.hip): a summed double-mask encrypt launch over clients a .. b also writes
D = term(b + 1) - term(a) of its elements, and a decrypt of the sum with exactly ([b + 1], [a]), iter, key, n and n_jobs on a range
inside the covered one is a combine with D instead of two more AES streams.  Every decrypt here -- fast path or fall-back -- is
compared with the CPU oracle's decrypt of the same (device-computed) sum, into output buffers poisoned before every call.

The summed launch only runs when the vector gives every wave of the chip two whole tiles (launch_prf_batch_sum), so the vectors
here are a few million elements long."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
KEY = bytes(range(32))
KEY2 = bytes(range(100, 132))
J = 16


@pytest.fixture(scope="module")
def E():
    from flashe_amd import engine
    return engine


def _poison(eng, buf, byte=0x3C):
    eng.memset_dev(buf, byte, buf.nbytes)


def _summed_round(E, eng, it, idx, n, seed):
    """C encrypts as one summed chain (the call bench.py times); returns (device sum, host sum)."""
    pts = [np.random.Generator(np.random.PCG64(seed + c)).integers(0, 2 ** 64, n, dtype=np.uint64) for c in range(len(idx))]
    dpt = [eng.upload(p) for p in pts]
    dct = [eng.alloc_vec(n) for _ in idx]
    dsum = eng.alloc_vec(n)
    _poison(eng, dsum, 0xA5)
    eng.encrypt_batch_sum_dev(it, list(idx), E.SCHEME_DOUBLE, n, J, dpt, 1, dct, dsum)
    return dsum, dsum.download(np.uint64, 2 * n).reshape(n, 2)


def _decrypt(eng, it, add, minus, n, n_jobs, first, count, dsum, dout):
    _poison(eng, dout)
    eng.decrypt_range_dev(it, add, minus, n, n_jobs, first, count, dsum.ptr + 16 * first, dout.ptr + 16 * first)
    return dout.download(np.uint64, 2 * n).reshape(n, 2)[first:first + count]


@pytest.mark.parametrize("b", [128, 100])
@pytest.mark.parametrize("n", [2_621_440, 2_600_037])          # whole tiles, ragged
def test_fast_path_full_and_sub_ranges(E, oracle, b, n):
    eng = E.Engine(KEY, b, device=0)
    it, idx = 7, [2, 3, 4]
    dsum, hsum = _summed_round(E, eng, it, idx, n, 100 + b)
    want = oracle.decrypt(KEY, it, [5], [2], J, b, hsum)
    dout = eng.alloc_vec(n)
    for first, count in [(0, n), (0, 1000), (n // 3 + 17, n // 4), (n - 999, 999), (255, 1)]:
        got = _decrypt(eng, it, [5], [2], n, J, first, count, dsum, dout)
        assert np.array_equal(got, want[first:first + count]), (first, count)
    # the slot is not consumed: the same decrypt again, in place
    eng.decrypt_range_dev(it, [5], [2], n, J, 0, n, dsum, dsum)
    assert np.array_equal(dsum.download(np.uint64, 2 * n).reshape(n, 2), want)


def test_range_encrypt_fills_its_range(E, oracle):
    """flashe_encrypt_batch_range_dev with a sum (element sharding): the mask covers [first, first + count) only."""
    b, n, F, CNT, it, idx = 128, 3_000_000, 300_001, 2_400_000, 4, [0, 1, 2, 3]
    eng = E.Engine(KEY, b, device=0)
    pts = [np.random.Generator(np.random.PCG64(40 + c)).integers(0, 2 ** 64, n, dtype=np.uint64) for c in idx]
    dpt = [eng.upload(p) for p in pts]
    dct = [eng.alloc_vec(n) for _ in idx]
    dsum = eng.alloc_vec(n)
    _poison(eng, dsum, 0xA5)
    eng.encrypt_batch_range_dev(it, idx, E.SCHEME_DOUBLE, n, J, F, CNT, [d.ptr + 8 * F for d in dpt], 1,
                                [d.ptr + 16 * F for d in dct], dsum.ptr + 16 * F)
    hsum = dsum.download(np.uint64, 2 * n).reshape(n, 2)
    want = oracle.decrypt(KEY, it, [4], [0], J, b, hsum)
    dout = eng.alloc_vec(n)
    for first, count in [(F, CNT), (F + 12_345, 1_000_000), (F + CNT - 7, 7),        # inside: the mask
                         (F - 1, 10), (F + CNT - 5, 10), (0, n)]:                   # reaching outside: the PRF path
        got = _decrypt(eng, it, [4], [0], n, J, first, count, dsum, dout)
        assert np.array_equal(got, want[first:first + count]), (first, count)
    lo = sum(p.astype(object) for p in pts)                                         # (and the round trip on the covered range)
    got = _decrypt(eng, it, [4], [0], n, J, F, CNT, dsum, dout)
    assert [int(got[k, 0]) | (int(got[k, 1]) << 64) for k in (0, CNT // 2, CNT - 1)] == [int(lo[F + k]) for k in (0, CNT // 2, CNT - 1)]


def test_mismatched_keys_fall_back(E, oracle):
    """Another iter, another (add, minus) pair (a dropout list), other n_jobs, another n: the PRF path, still exact."""
    b, n, it, idx = 128, 2_600_037, 9, [0, 1, 2, 3, 4]
    eng = E.Engine(KEY, b, device=0)
    dsum, hsum = _summed_round(E, eng, it, idx, n, 300)
    dout = eng.alloc_vec(n)
    add, minus = E.telescope([0, 1, 3, 4])                                           # a dropout: two runs
    for it2, a, m, nj in [(it + 1, [5], [0], J), (it, add, minus, J), (it, [5], [1], J), (it, [4], [0], J), (it, [5], [0], 7)]:
        want = oracle.decrypt(KEY, it2, a, m, nj, b, hsum)
        assert np.array_equal(_decrypt(eng, it2, a, m, n, nj, 0, n, dsum, dout), want), (it2, a, m, nj)
    # another n (int_bits > 64: the streams do not depend on n, so the oracle's decrypt of the same elements is the reference)
    want = oracle.decrypt(KEY, it, [5], [0], J, b, hsum)
    _poison(eng, dout)
    eng.decrypt_range_dev(it, [5], [0], n + 4, J, 0, n, dsum, dout)
    assert np.array_equal(dout.download(np.uint64, 2 * n).reshape(n, 2), want)
    # and the fast path is still right after all of those
    assert np.array_equal(_decrypt(eng, it, [5], [0], n, J, 0, n, dsum, dout), want)


def test_set_key_invalidates(E, oracle):
    b, n, it, idx = 128, 2_600_037, 3, [0, 1, 2]
    eng = E.Engine(KEY, b, device=0)
    dsum, hsum = _summed_round(E, eng, it, idx, n, 500)
    dout = eng.alloc_vec(n)
    eng.set_key(KEY2)
    assert np.array_equal(_decrypt(eng, it, [3], [0], n, J, 0, n, dsum, dout), oracle.decrypt(KEY2, it, [3], [0], J, b, hsum))
    eng.set_key(KEY)                                                                 # back to the first key: the slot stays invalid
    assert np.array_equal(_decrypt(eng, it, [3], [0], n, J, 0, n, dsum, dout), oracle.decrypt(KEY, it, [3], [0], J, b, hsum))


def test_second_summed_launch_replaces_the_slot(E, oracle):
    b, n, idx = 128, 2_600_037, [0, 1, 2]
    eng = E.Engine(KEY, b, device=0)
    dsum1, hsum1 = _summed_round(E, eng, 5, idx, n, 600)
    dsum2, hsum2 = _summed_round(E, eng, 6, idx, n, 700)
    dout = eng.alloc_vec(n)
    assert np.array_equal(_decrypt(eng, 5, [3], [0], n, J, 0, n, dsum1, dout), oracle.decrypt(KEY, 5, [3], [0], J, b, hsum1))
    assert np.array_equal(_decrypt(eng, 6, [3], [0], n, J, 0, n, dsum2, dout), oracle.decrypt(KEY, 6, [3], [0], J, b, hsum2))


def test_graph_capture_and_replay_invalidate(E, oracle):
    """A summed launch captured into a graph writes no mask; the capture and every replay (the iter-shift word) invalidate the slot."""
    b, n, it, idx = 128, 2_600_037, 11, [0, 1, 2]
    eng = E.Engine(KEY, b, device=0)
    pts = [np.random.Generator(np.random.PCG64(800 + c)).integers(0, 2 ** 64, n, dtype=np.uint64) for c in idx]
    dpt = [eng.upload(p) for p in pts]
    dct = [eng.alloc_vec(n) for _ in idx]
    dsum, dout = eng.alloc_vec(n), eng.alloc_vec(n)
    eng.encrypt_batch_sum_dev(it, idx, E.SCHEME_DOUBLE, n, J, dpt, 1, dct, dsum)   # eager: fills the slot for iter `it`
    eng.sync()
    eng.graph_begin()
    eng.encrypt_batch_sum_dev(it, idx, E.SCHEME_DOUBLE, n, J, dpt, 1, dct, dsum)
    g = eng.graph_end()
    _poison(eng, dsum, 0xA5)
    g.launch(iter_shift=1)                                                           # the round at it + 1
    hsum = dsum.download(np.uint64, 2 * n).reshape(n, 2)
    for it2 in (it + 1, it):
        assert np.array_equal(_decrypt(eng, it2, [3], [0], n, J, 0, n, dsum, dout), oracle.decrypt(KEY, it2, [3], [0], J, b, hsum)), it2
    _poison(eng, dsum, 0xA5)
    g.launch()                                                                       # the captured round again (iter `it`)
    hsum = dsum.download(np.uint64, 2 * n).reshape(n, 2)
    assert np.array_equal(_decrypt(eng, it, [3], [0], n, J, 0, n, dsum, dout), oracle.decrypt(KEY, it, [3], [0], J, b, hsum))


def test_decrypt_on_another_ctx(E, oracle):
    b, n, it, idx = 128, 2_600_037, 2, [0, 1, 2]
    eng = E.Engine(KEY, b, device=0)
    dsum, hsum = _summed_round(E, eng, it, idx, n, 900)
    side = E.Engine(KEY, b, device=0)
    dout = side.alloc_vec(n)
    _poison(side, dout)
    side.decrypt_range_dev(it, [3], [0], n, J, 0, n, dsum, dout)
    want = oracle.decrypt(KEY, it, [3], [0], J, b, hsum)
    assert np.array_equal(dout.download(np.uint64, 2 * n).reshape(n, 2), want)
    assert np.array_equal(_decrypt(eng, it, [3], [0], n, J, 0, n, dsum, eng.alloc_vec(n)), want)


def test_option_off(E, oracle, monkeypatch):
    """FLASHE_CHAIN_DMASK=0 (read at ctx creation): the summed launch writes no mask, the decrypt computes its streams."""
    monkeypatch.setenv("FLASHE_CHAIN_DMASK", "0")
    b, n, it, idx = 128, 2_600_037, 8, [1, 2, 3]
    eng = E.Engine(KEY, b, device=0)
    dsum, hsum = _summed_round(E, eng, it, idx, n, 1000)
    dout = eng.alloc_vec(n)
    assert np.array_equal(_decrypt(eng, it, [4], [1], n, J, 0, n, dsum, dout), oracle.decrypt(KEY, it, [4], [1], J, b, hsum))


def test_explicit_prepared_decrypt_survives(E, oracle):
    b, n, it = 128, 2_600_037, 12
    eng = E.Engine(KEY, b, device=0)
    eng.prepare_decrypt(it, 3, n, J)
    assert eng.prepared_query(eng.PREPARED_DECRYPT)[0]
    dsum, hsum = _summed_round(E, eng, it, [0, 1, 2], n, 1100)
    assert eng.prepared_query(eng.PREPARED_DECRYPT)[0], "the summed launch must not touch flashe_prepare_decrypt's slot"
    dout = eng.alloc_vec(n)
    assert np.array_equal(_decrypt(eng, it, [3], [0], n, J, 0, n, dsum, dout), oracle.decrypt(KEY, it, [3], [0], J, b, hsum))
