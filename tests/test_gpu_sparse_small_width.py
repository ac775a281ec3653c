"""GPU tests of the sparse single-mask passes with the PRF inside at int_bits <= 64 (span_prf_small_kernel, stream.hip): the one-limb
widths the reference's sparse jobs run at (int_bits 20).  Entry q of client c's k-entry list is slot (q - begin) % m of the block
AES(key, iter | idx[c] | begin + (q - begin) / m) of its chunk [begin, end) of chunks_idx(range(k), n_jobs), m = 128 / b
(jzf_flashe.py:19-45, :316-343, :471-478, :531-532; jzf_aggregator.py:150-165, :419-430).  Every output is compared with the CPU
oracle, written into buffers poisoned with a byte pattern first."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEY = bytes(range(32))
SPAN = 1752
POISON = 0xa5
POISON64 = np.uint64(0xa5a5a5a5a5a5a5a5)


@pytest.fixture(scope="module")
def E():
    from flashe_amd import engine
    return engine


def make(E, b):
    return E.Engine(KEY, b, device=0)


def bmask(b):
    return np.uint64((1 << b) - 1) if b < 64 else np.uint64(2 ** 64 - 1)


def lists(rng, total, ks):
    return [np.sort(rng.choice(total, kc, replace=False)).astype(np.uint32) for kc in ks]


def ragged(rng, C, total, J):
    """list lengths: every position, none, one, fewer than n_jobs, n_jobs + 1, and random ones around 1 - 30 %"""
    fixed = [total, 0, 1, max(J - 1, 0), min(J + 1, total), min(2 * J + 3, total)]
    ks = fixed[:C] + [int(rng.integers(0, max(total * 3 // 10, 2))) for _ in range(C - len(fixed[:C]))]
    return [min(k, total) for k in ks]


def oracle_round(oracle, it, idx, locs, pts, zeros, total, J, b):
    """every client's compact ciphertext and the aggregate of the expanded uploads (sum_c zero_c + (ct - zero_c) at its positions)"""
    m = bmask(b)
    cts = [oracle.encrypt(KEY, it, i, "single", J, b, p)[:, 0] if len(p) else np.zeros(0, dtype=np.uint64) for i, p in zip(idx, pts)]
    agg = np.full(total, np.uint64(sum(zeros) % (1 << 64)), dtype=np.uint64)
    with np.errstate(over="ignore"):
        for l, ct, z in zip(locs, cts, zeros):
            agg[l] += ct - np.uint64(z)
    return cts, agg & m


def upload_all(eng, arrs):
    return [eng.upload(a) if a.size else eng.alloc(16) for a in arrs]


def poisoned(eng, n):
    buf = eng.alloc_vec(max(n, 1))
    eng.memset_dev(buf, POISON, buf.nbytes)
    return buf


ENC_SHAPES = [(5, 1_752), (70, 1_753), (3, 1_751), (6, 1_752 * 7 + 1), (4, 1_752 * 9 - 1), (8, 1_752 * 3)]
ENC_CASES = [(b, J, ENC_SHAPES[(i * 3 + j) % len(ENC_SHAPES)]) for i, b in enumerate((1, 7, 16, 20, 23, 32, 33, 63, 64))
             for j, J in enumerate((1, 16, 40))]


@pytest.mark.parametrize("b,J,shape", ENC_CASES, ids=[f"b{b}-J{J}-C{s[0]}-n{s[1]}" for b, J, s in ENC_CASES])
def test_encrypt_aggregate_one_limb(E, oracle, b, J, shape):
    """flashe_sparse_encrypt_aggregate_dev at int_bits <= 64: every client's ciphertext and the aggregate, with and without a bounds
    handle, and as ONE position range over the whole vector (flashe_sparse_encrypt_aggregate_range_dev: the pass with the PRF inside);
    ragged lists (empty, every position, fewer entries than chunks), client indices other than 0 .. C-1, two groups at C = 70."""
    C, total = shape
    eng = make(E, b)
    rng = np.random.Generator(np.random.PCG64(b * 100 + J + C))
    ks = ragged(rng, C, total, J)
    locs = lists(rng, total, ks)
    pts = [rng.integers(0, 2 ** b, kc, dtype=np.uint64) for kc in ks]
    idx = [(7 * c + 3) % 251 for c in range(C)]
    zeros = [(c * 12345 + 7) & ((1 << b) - 1) for c in range(C)]
    want_ct, want_agg = oracle_round(oracle, 6, idx, locs, pts, zeros, total, J, b)
    dl, dp = upload_all(eng, locs), upload_all(eng, pts)
    for form in ("whole", "bounds", "range"):
        bnd = eng.span_bounds(total, dl, ks) if form != "whole" else None
        cts = [poisoned(eng, kc) for kc in ks]
        agg = poisoned(eng, total)
        eng.sparse_encrypt_aggregate_dev(6, idx, dl, ks, dp, 1, zeros, total, J, cts, agg, bounds=bnd,
                                         position_range=(0, total) if form == "range" else None)
        for c in range(C):
            got = cts[c].download(np.uint64, max(ks[c], 1))
            assert np.array_equal(got[:ks[c]], want_ct[c]), (b, J, C, total, c, form, "ciphertext")
        assert np.array_equal(agg.download(np.uint64, total), want_agg), (b, J, C, total, form, "aggregate")


@pytest.mark.parametrize("b", [1, 7, 20, 33, 64])
@pytest.mark.parametrize("J", [1, 16, 40])
def test_decrypt_one_limb(E, oracle, b, J):
    """flashe_sparse_decrypt_dev (sorted and unsorted lists) and flashe_sparse_decrypt_bounds_dev equal combine(agg, -sparse_minus_mask);
    the bounds form was refused at int_bits <= 64 before."""
    eng = make(E, b)
    rng = np.random.Generator(np.random.PCG64(700 + b + J))
    C, total = (70, 1_752 * 3 + 11) if J == 16 else (6, 1_752 * 5 - 3)
    ks = ragged(rng, C, total, J)
    locs = lists(rng, total, ks)
    agg_h = rng.integers(0, 2 ** b, total, dtype=np.uint64)
    want = oracle.combine(b, agg_h.reshape(total, 1), None, oracle.sparse_minus_mask(KEY, 8, locs, total, J, b))[:, 0]
    dl = upload_all(eng, locs)
    agg = eng.upload(agg_h)
    bnd = eng.span_bounds(total, dl, ks)
    for form in ("sorted", "unsorted", "bounds"):
        out = poisoned(eng, total)
        if form == "bounds":
            eng.sparse_decrypt_dev(8, dl, ks, total, J, agg, out, bounds=bnd)
        else:
            eng.sparse_decrypt_dev(8, dl, ks, total, J, agg, out, sorted_lists=(form == "sorted"))
        assert np.array_equal(out.download(np.uint64, total), want), (b, J, form)
    assert np.array_equal(agg.download(np.uint64, total), agg_h)


@pytest.mark.parametrize("b", [7, 20, 64])
@pytest.mark.parametrize("parts", [3, 5, 8])
def test_position_ranges_one_limb(E, oracle, b, parts):
    """flashe_sparse_encrypt_aggregate_range_dev / flashe_sparse_decrypt_range_dev at int_bits <= 64: span-aligned parts laid side by
    side equal the whole-vector calls and the oracle; a range writes exactly the ciphertext entries whose position it owns (the rest keep
    the poison); misaligned ranges are refused."""
    from flashe_amd._lib import FlasheError
    eng = make(E, b)
    J = 16
    rng = np.random.Generator(np.random.PCG64(900 + b + parts))
    C, total = 7, 1_752 * 11 + 5
    ks = ragged(rng, C, total, J)
    locs = lists(rng, total, ks)
    pts = [rng.integers(0, 2 ** b, kc, dtype=np.uint64) for kc in ks]
    idx = [(5 * c + 2) % 89 for c in range(C)]
    zeros = [3 + c for c in range(C)]
    want_ct, want_agg = oracle_round(oracle, 4, idx, locs, pts, zeros, total, J, b)
    want_dec = oracle.combine(b, want_agg.reshape(total, 1), None, oracle.sparse_minus_mask(KEY, 4, locs, total, J, b))[:, 0]
    dl, dp = upload_all(eng, locs), upload_all(eng, pts)
    bnd = eng.span_bounds(total, dl, ks)
    n_spans = (total + SPAN - 1) // SPAN
    edges = [min(total, SPAN * ((n_spans * g) // parts)) for g in range(parts)] + [total]
    cts = [poisoned(eng, kc) for kc in ks]
    got_agg, got_dec = np.zeros(total, dtype=np.uint64), np.zeros(total, dtype=np.uint64)
    for g in range(parts):
        first, count = edges[g], edges[g + 1] - edges[g]
        sl_a, sl_d = poisoned(eng, count), poisoned(eng, count)
        eng.sparse_encrypt_aggregate_dev(4, idx, dl, ks, dp, 1, zeros, total, J, cts, sl_a, bounds=bnd, position_range=(first, count))
        eng.sparse_decrypt_dev(4, dl, ks, total, J, sl_a, sl_d, bounds=bnd, position_range=(first, count))
        got_agg[first:first + count] = sl_a.download(np.uint64, max(count, 1))[:count]
        got_dec[first:first + count] = sl_d.download(np.uint64, max(count, 1))[:count]
        for c in range(C):
            have = cts[c].download(np.uint64, max(ks[c], 1))[:ks[c]]
            done = locs[c] < edges[g + 1]
            assert np.array_equal(have[done], want_ct[c][done]) and np.all(have[~done] == POISON64), (b, parts, g, c)
    assert np.array_equal(got_agg, want_agg), (b, parts, "aggregate")
    assert np.array_equal(got_dec, want_dec), (b, parts, "decrypt")
    out = poisoned(eng, total)
    for bad in ((5, SPAN), (0, SPAN + 1), (SPAN, 2 * SPAN - 1)):
        with pytest.raises(FlasheError):
            eng.sparse_decrypt_dev(4, dl, ks, total, J, eng.upload(want_agg), out, bounds=bnd, position_range=bad)
        with pytest.raises(FlasheError):
            eng.sparse_encrypt_aggregate_dev(4, idx, dl, ks, dp, 1, zeros, total, J, cts, out, bounds=bnd, position_range=bad)


def test_span_prf_small_crowded_dense_sparse_and_empty_spans(E, oracle):
    """The int_bits = 20 counterpart of test_span_prf_crowded_dense_sparse_and_empty_spans: ~1,500 spans, six per workgroup, whose
    density changes from span to span -- crowded (more blocks than lanes), one client holding every position, the usual 1 %, empty --
    over three rounds back to back; every ciphertext, the aggregate and the decrypted vector against the oracle."""
    b, J, C = 20, 16, 6
    eng = make(E, b)
    n_spans = 6 * 256 + 3
    total = SPAN * n_spans - 7
    rng = np.random.Generator(np.random.PCG64(2020))
    mode = np.arange(n_spans) % 5
    dens = np.array([[0.30, 0.30, 0.25, 0.02, 0.0, 0.01],
                     [0.01, 0.01, 0.01, 0.01, 0.01, 0.01],
                     [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                     [1.0, 0.01, 0.0, 0.2, 0.0, 0.01],
                     [0.05, 0.0, 0.0, 0.0, 0.6, 0.0]])
    p_of_pos = dens[np.repeat(mode, SPAN)[:total]]
    locs = [np.flatnonzero(rng.random(total) < p_of_pos[:, c]).astype(np.uint32) for c in range(C)]
    ks = [int(l.size) for l in locs]
    assert max(ks) > 300_000 and min(ks) > 10_000
    idx = [7, 8, 30, 2, 0, 55]
    zeros = [1 << 19, 5, 3, 0, 77, (1 << 20) - 1]
    dl = upload_all(eng, locs)
    bnd = eng.span_bounds(total, dl, ks)
    agg, dec = eng.alloc_vec(total), eng.alloc_vec(total)
    for it in (3, 4, 5):
        pts = [rng.integers(0, 2 ** b, kc, dtype=np.uint64) for kc in ks]
        dp = upload_all(eng, pts)
        cts = [poisoned(eng, kc) for kc in ks]
        for buf in (agg, dec):
            eng.memset_dev(buf, POISON, buf.nbytes)
        eng.sparse_encrypt_aggregate_dev(it, idx, dl, ks, dp, 1, zeros, total, J, cts, agg, bounds=bnd)
        eng.sparse_decrypt_dev(it, dl, ks, total, J, agg, dec, sorted_lists=True, bounds=bnd)
        want_ct, want_agg = oracle_round(oracle, it, idx, locs, pts, zeros, total, J, b)
        for c in range(C):
            assert np.array_equal(cts[c].download(np.uint64, ks[c]), want_ct[c]), (it, c, "ciphertext")
        assert np.array_equal(agg.download(np.uint64, total), want_agg), (it, "aggregate")
        mask = oracle.sparse_minus_mask(KEY, it, locs, total, J, b)
        assert np.array_equal(dec.download(np.uint64, total), oracle.combine(b, want_agg.reshape(total, 1), None, mask)[:, 0]), (it, "decrypt")


@pytest.mark.parametrize("world", [2, 3])
def test_sparse_sharded_round_small_width_several_ranks(world, tmp_path):
    """flashe_amd.dist.SparseShardedRound at int_bits = 20 (it raised ValueError before) with real kernels and `world` ranks sharing
    device 0, the exchange through tests/shm_comm.py: the gathered round trip is the plain sparse sum, every rank's ciphertext entries
    are the whole-list encrypt's."""
    from conftest import ROOT
    from shm_comm import launch_ranks
    outs = launch_ranks(os.path.join(ROOT, "tests", "dist_gpu_sparse_small_worker.py"), world, tmp_path, timeout=900)
    for p, (rc, so, se) in enumerate(outs):
        assert rc == 0, f"process {p}: {so[-1500:]}{se[-3000:]}"
    assert "DIST_GPU_SPARSE_SMALL_OK" in outs[0][1]
