"""The element-wise model of tests/elementwise_ref.py checked against what comes from the reference (the golden mask streams) and
against the CPU oracle's whole-vector streams, and the host chunking (flashe_chunks) against the model's chunk formula at the
sizes where 32-bit arithmetic would break.  The GPU tests of tests/test_gpu_index_limits.py take the model as their expected value."""
import numpy as np
import pytest

import elementwise_ref as ref
from conftest import load_golden, unhex

KEY = bytes(range(32))


def test_model_matches_golden_mask_streams():
    g = load_golden("mask_streams.json")
    key = bytes.fromhex(g["key"])
    assert len(g["cases"]) == 116
    for c in g["cases"]:
        b, n, J = c["b"], c["n"], c["n_jobs"]
        assert [list(x) for x in ref.chunk_bounds(n, J)] == c["chunks"], (n, J)
        got = ref.mask(key, c["iter"], [c["idx"]], n, J, b, range(n))
        assert got == unhex(c["stream"]), (b, n, J)
    for c in g["sums"]:
        b, n, J = c["b"], c["n"], c["n_jobs"]
        assert ref.mask(key, c["iter"], c["add_idx"], n, J, b, range(n)) == unhex(c["add"])
        assert ref.mask(key, c["iter"], c["minus_idx"], n, J, b, range(n)) == unhex(c["minus"])


@pytest.mark.parametrize("J", [1, 3, 16, 17])
def test_model_matches_oracle_streams(oracle, J):
    """Every width 1..128 (the non-divisors of 128 leave unused bits at the top of each block) at n on both sides of n_jobs."""
    it, idx = 11, 6
    for b in range(1, 129):
        n = (b * 7 + J) % 61 + 1
        want = oracle.limbs_to_ints(oracle.mask(KEY, it, idx, n, J, b))
        assert ref.mask(KEY, it, [idx], n, J, b, range(n)) == want, (b, n, J)


@pytest.mark.parametrize("b", [1, 7, 20, 33, 64, 100, 128])
def test_model_encrypt_decrypt_match_oracle(oracle, b):
    rng = np.random.Generator(np.random.PCG64(b))
    n, J, it = 257, 17, 4
    pt = rng.integers(0, 2 ** 63, n, dtype=np.uint64).reshape(-1, 1)
    for double in (False, True):
        want = oracle.limbs_to_ints(oracle.encrypt(KEY, it, 9, "double" if double else "single", J, b, pt))
        assert ref.encrypt(KEY, it, 9, double, n, J, b, range(n), pt[:, 0]) == want, (b, double)
    ct = oracle.ints_to_limbs([int(v) for v in rng.integers(0, 2 ** 63, n, dtype=np.uint64)], b)
    want = oracle.limbs_to_ints(oracle.decrypt(KEY, it, [3, 8], [0, 5, 7], J, b, ct))
    assert ref.decrypt(KEY, it, [3, 8], [0, 5, 7], n, J, b, range(n), oracle.limbs_to_ints(ct)) == want


@pytest.mark.parametrize("b", [1, 20, 64, 65, 128])
@pytest.mark.parametrize("J", [1, 16])
def test_model_sparse_minus_mask_matches_oracle(oracle, b, J):
    rng = np.random.Generator(np.random.PCG64(1000 * b + J))
    total, it = 3000, 8
    locs = [np.sort(rng.choice(total, size=k, replace=False)).astype(np.uint32) for k in (0, 1, 700, 1300, 2999)]
    want = oracle.limbs_to_ints(oracle.sparse_minus_mask(KEY, it, locs, total, J, b))
    assert ref.sparse_minus_mask(KEY, it, locs, J, b, range(total)) == want


@pytest.mark.parametrize("n", [2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 3])
@pytest.mark.parametrize("J", [1, 3, 16, 17])
def test_host_chunks_beyond_32_bits(n, J):
    from flashe_amd import engine
    b = engine.chunks(n, J)
    assert [(b[i], b[i + 1]) for i in range(J)] == list(ref.chunk_bounds(n, J))
    d, r = divmod(n, J)
    assert all(e - s == (d + 1 if c < r else d) for c, (s, e) in enumerate(ref.chunk_bounds(n, J)))


def test_model_terms_beyond_2_32():
    """Elements above 2^32: the model reads the 8-byte counter big-endian, high word first (the block input of
    jzf_flashe.py:34), which a 32-bit counter would lose."""
    n, J, b, it, idx = 2 ** 40 + 3, 1, 64, 2, 5
    j = 2 ** 33 + 5                        # one chunk: block (j // 2), slot 1
    S = int.from_bytes(ref.flashe_oracle.aes256_encrypt_block(KEY, it.to_bytes(4, "big") + idx.to_bytes(4, "big")
                                                              + (j // 2).to_bytes(8, "big")), "big")
    assert ref.term(KEY, it, idx, n, J, b, j) == S >> 64
    assert ref.term(KEY, it, idx, n, J, b, j) != ref.term(KEY, it, idx, n, J, b, j - 2 ** 33)
