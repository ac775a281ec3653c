"""flashe_encrypt_batch_sum_decrypt_dev: the round of a device that plays the clients and the arbiter -- the ciphertexts, their sum and the
decrypt of the sum.  At int_bits 128 with one-limb plaintexts on a vector that gives every wave two whole tiles it is ONE launch
(prf_dec_sum128_kernel stores sum + D where prf_dmask_sum128_kernel stores D); every other shape, and FLASHE_CHAIN_DEC=0, is
flashe_encrypt_batch_sum_dev followed by flashe_decrypt_dev.  Every output of every case -- each ciphertext, the sum, the decrypt -- is
compared bit for bit with the CPU oracle, with the plain sum of the plaintexts, and with the two calls run on a second set of buffers;
all outputs are poisoned with distinct bytes before each call.

T = 2 x CUs x 16 tiles of 256 elements is the admission bound of the summed launch (launch_prf_batch_sum), so the vectors are about two
million elements long."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
KEY = bytes(range(32))
EINVAL = -22


@pytest.fixture(scope="module")
def E():
    from flashe_amd import engine
    return engine


def _tiles(eng):
    return 2 * eng.cu_count * 16


def _plain_sum(pts, b):
    """sum of the plaintexts mod 2^b as [n, 2] limbs; pts: [n] (one limb) or [n, 2]."""
    n = pts[0].shape[0]
    lo, hi = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    for p in pts:
        p = p.reshape(n, -1)
        new = lo + p[:, 0]
        hi += (new < lo).astype(np.uint64)
        if p.shape[1] == 2:
            hi += p[:, 1]
        lo = new
    if b < 128:
        hi &= np.uint64((1 << (b - 64)) - 1)
    return np.stack([lo, hi], axis=1)


def _buffers(eng, C, n):
    """ct, sum, dec of one call, poisoned with distinct bytes"""
    cts, dsum, ddec = [eng.alloc_vec(n) for _ in range(C)], eng.alloc_vec(n), eng.alloc_vec(n)
    for c, buf in enumerate(cts):
        eng.memset_dev(buf, 0x91 + c, buf.nbytes)
    eng.memset_dev(dsum, 0xA5, dsum.nbytes)
    eng.memset_dev(ddec, 0x3C, ddec.nbytes)
    return cts, dsum, ddec


def _host(buf, n):
    return buf.download(np.uint64, 2 * n).reshape(n, 2)


def _check_round(E, oracle, eng, b, it, idx, n, n_jobs, pt_limbs=1, seed=0):
    C = len(idx)
    rng = np.random.Generator(np.random.PCG64(seed))
    pts = [rng.integers(0, 2 ** 64, n if pt_limbs == 1 else (n, 2), dtype=np.uint64) for _ in range(C)]
    if pt_limbs == 2 and b < 128:
        for p in pts:
            p[:, 1] &= np.uint64((1 << (b - 64)) - 1)
    dpt = [eng.upload(p) for p in pts]
    cts, dsum, ddec = _buffers(eng, C, n)
    eng.encrypt_batch_sum_decrypt_dev(it, idx, E.SCHEME_DOUBLE, n, n_jobs, dpt, pt_limbs, cts, dsum, ddec)
    cts2, dsum2, ddec2 = _buffers(eng, C, n)
    eng.encrypt_batch_sum_dev(it, idx, E.SCHEME_DOUBLE, n, n_jobs, dpt, pt_limbs, cts2, dsum2)
    eng.decrypt_dev(it, [idx[-1] + 1], [idx[0]], n, n_jobs, dsum2, ddec2)
    want_sum = np.zeros((n, 2), dtype=np.uint64)
    for c in range(C):
        want = oracle.encrypt(KEY, it, idx[c], "double", n_jobs, b, pts[c])
        got = _host(cts[c], n)
        assert np.array_equal(got, want), ("ct", c)
        assert np.array_equal(got, _host(cts2[c], n)), ("ct against the two calls", c)
        want_sum = oracle.aggregate_elem([want_sum, want], b)
    got_sum, got_dec = _host(dsum, n), _host(ddec, n)
    assert np.array_equal(got_sum, want_sum), "sum"
    assert np.array_equal(got_dec, oracle.decrypt(KEY, it, [idx[-1] + 1], [idx[0]], n_jobs, b, want_sum)), "decrypt of the sum"
    assert np.array_equal(got_dec, _plain_sum(pts, b)), "the plaintexts' sum"
    assert np.array_equal(got_sum, _host(dsum2, n)) and np.array_equal(got_dec, _host(ddec2, n)), "against the two calls"


@pytest.mark.parametrize("shape, C, n_jobs", [("whole", 1, 16), ("edge", 2, 16), ("leftover", 3, 16), ("leftover", 3, 5)])
def test_one_launch_shapes(E, oracle, shape, C, n_jobs):
    """whole: all whole tiles, the last stream is the first link.  edge: the last tile holds ONE element, at the admission limit.
    leftover: every workgroup has one tile more than its waves share evenly (the half-tile store site) and a ragged end."""
    eng = E.Engine(KEY, 128, device=0)
    T = _tiles(eng)
    n = {"whole": 256 * T, "edge": 256 * T - 255, "leftover": 256 * (T + eng.cu_count) - 77}[shape]
    _check_round(E, oracle, eng, 128, 6, list(range(2, 2 + C)), n, n_jobs, seed=11 * C + n_jobs)


def test_one_launch_at_the_32_bit_limits(E, oracle):
    eng = E.Engine(KEY, 128, device=0)
    _check_round(E, oracle, eng, 128, 2 ** 32 - 1, [2 ** 32 - 4, 2 ** 32 - 3], 256 * _tiles(eng), 16, seed=3)


@pytest.mark.parametrize("case", ["short", "bits96", "two_limb_pt", "option_off"])
def test_two_call_shapes(E, oracle, monkeypatch, case):
    """What the one launch does not carry runs as the two calls: the same bytes."""
    if case == "option_off":
        monkeypatch.setenv("FLASHE_CHAIN_DEC", "0")           # read at ctx creation
    b = 96 if case == "bits96" else 128
    eng = E.Engine(KEY, b, device=0)
    n = 256 * _tiles(eng) - (256 if case == "short" else 0)
    _check_round(E, oracle, eng, b, 9, [0, 1], n, 16, pt_limbs=2 if case == "two_limb_pt" else 1, seed=40)


def test_argument_checks_write_nothing(E):
    from flashe_amd._lib import FlasheError
    eng = E.Engine(KEY, 128, device=0)
    n, idx = 256 * _tiles(eng), [0, 1]
    dpt = [eng.upload(np.full(n, 7 + c, dtype=np.uint64)) for c in idx]
    cts, dsum, ddec = _buffers(eng, 2, n)
    before = [_host(buf, n).copy() for buf in cts + [dsum, ddec]]
    for dec in (dsum, cts[0], ddec.ptr + 8, dpt[1]):
        with pytest.raises(FlasheError) as err:
            eng.encrypt_batch_sum_decrypt_dev(3, idx, E.SCHEME_DOUBLE, n, 16, dpt, 1, cts, dsum, dec)
        assert err.value.code == EINVAL
    with pytest.raises(FlasheError) as err:                    # the decrypt's add prefix idx + 1 = 2^32
        eng.encrypt_batch_sum_decrypt_dev(3, [2 ** 32 - 2, 2 ** 32 - 1], E.SCHEME_DOUBLE, n, 16, dpt, 1, cts, dsum, ddec)
    assert err.value.code == EINVAL
    for buf, want in zip(cts + [dsum, ddec], before):
        assert np.array_equal(_host(buf, n), want)


def test_empty_calls_as_the_two_calls(E):
    eng = E.Engine(KEY, 128, device=0)
    n = 1000
    cts, dsum, ddec = _buffers(eng, 1, n)
    poison = [_host(buf, n).copy() for buf in (cts[0], dsum, ddec)]
    eng.encrypt_batch_sum_decrypt_dev(1, [4], E.SCHEME_DOUBLE, 0, 16, [eng.upload(np.zeros(2, dtype=np.uint64))], 1, cts, dsum, ddec)
    for buf, want in zip((cts[0], dsum, ddec), poison):       # n = 0: nothing is written
        assert np.array_equal(_host(buf, n), want)
    eng.encrypt_batch_sum_decrypt_dev(1, [], E.SCHEME_DOUBLE, n, 16, [], 1, [], dsum, ddec)
    cts2, dsum2, ddec2 = _buffers(eng, 1, n)
    eng.encrypt_batch_sum_dev(1, [], E.SCHEME_DOUBLE, n, 16, [], 1, [], dsum2)
    eng.decrypt_dev(1, [], [], n, 16, dsum2, ddec2)
    assert np.array_equal(_host(dsum, n), _host(dsum2, n)) and not _host(dsum, n).any()          # n_vec = 0: the zero sum ...
    assert np.array_equal(_host(ddec, n), _host(ddec2, n)) and not _host(ddec, n).any()          # ... decrypted with empty lists


def test_sharded_round_one_rank(E, oracle):
    """ShardedRound(world 1).run(partial_agg=True): encrypt_phase asks for the decrypt with the encrypts, reduce_decrypt_phase hands it
    out -- for that `it` only; a skipped encrypt_phase still gets a real decrypt of self.partial."""
    from flashe_amd.dist import HipOps, ShardedRound
    eng = E.Engine(KEY, 128, device=0)
    ops = HipOps(eng)
    C, J = 3, 16
    n = 256 * (_tiles(eng) + eng.cu_count) - 77
    pts = [np.random.Generator(np.random.PCG64(70 + c)).integers(0, 2 ** 64, n, dtype=np.uint64) for c in range(C)]
    refs = [(ops.upload(p), 0) for p in pts]
    rnd = ShardedRound(ops, n, 128, list(range(C)), J, total_clients=C)
    plain = _plain_sum(pts, 128)
    want_sum = {}
    for it in (4, 5):
        for buf in (rnd.ct_all, rnd.partial, rnd.result):
            eng.memset_dev(buf, 0xB6, buf.nbytes)
        out = rnd.run(it, refs, 1, partial_agg=True)
        want_sum[it] = np.zeros((n, 2), dtype=np.uint64)
        for c in range(C):
            want = oracle.encrypt(KEY, it, c, "double", J, 128, pts[c])
            assert np.array_equal(ops.read(rnd.ct[c], 2 * n).reshape(n, 2), want), (it, c)
            want_sum[it] = oracle.aggregate_elem([want_sum[it], want], 128)
        assert np.array_equal(ops.read((rnd.partial, 0), 2 * n).reshape(n, 2), want_sum[it]), it
        got = ops.read((out, 0), 2 * n).reshape(n, 2)
        assert np.array_equal(got, oracle.decrypt(KEY, it, [C], [0], J, 128, want_sum[it])) and np.array_equal(got, plain), it
    # the note is good for one call: a second reduce_decrypt_phase of the same round decrypts self.partial for real
    eng.memset_dev(rnd.result, 0xB6, rnd.result.nbytes)
    out = rnd.reduce_decrypt_phase(5, partial_agg=True)
    assert np.array_equal(ops.read((out, 0), 2 * n).reshape(n, 2), plain)
    # encrypt_phase replaced by a no-op on a prepared partial (round 4's sum, after a real encrypt_phase of round 5 left its note): the
    # decrypt of THAT vector
    rnd.encrypt_phase(5, refs, 1, partial_agg=True)
    rnd.encrypt_phase = lambda *a, **k: None
    eng.memset_dev(rnd.result, 0xB6, rnd.result.nbytes)
    rnd.partial.upload(want_sum[4])
    out = rnd.run(4, refs, 1, partial_agg=True)
    assert np.array_equal(ops.read((out, 0), 2 * n).reshape(n, 2), plain)
