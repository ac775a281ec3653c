"""The helper of the wire kernels' GPU tests (tests/wire_ref.py) against itself and the CPU oracle.  No GPU.

weights.to_big_int / TransferableWeights pack on the device even for host arrays (the engine has no CPU fallback), so the comparison with
them is a GPU test (tests/test_gpu_wire_edges.py, the same lengths and widths); here the integer is held against the sum written out as
jzf_weights.py `_to_bytes_old` has it and against the oracle's pack, the host twin of what to_big_int runs."""
import numpy as np
import pytest

import wire_ref as W

LENGTHS = (1, 5, 129)
WIDTHS = (16, 17, 43, 64)


def _values(n, b):
    rng = np.random.Generator(np.random.PCG64(100 * b + n))
    vals = [int(v) for v in rng.integers(0, (1 << b) - 1, n, dtype=np.uint64, endpoint=True)]
    vals[-1] |= 1                                                           # the integer's lowest bit and its top bit are set
    vals[0] = (1 << b) - 1
    return vals


@pytest.mark.parametrize("b", WIDTHS)
@pytest.mark.parametrize("n", LENGTHS)
def test_wire_int_is_the_sum_compress_builds(oracle, n, b):
    vals = _values(n, b)
    big = W.wire_int(vals, b)
    assert big == sum(v << (b * (n - 1 - j)) for j, v in enumerate(vals))
    assert big.bit_length() == n * b and big & 1
    assert [(big >> (b * (n - 1 - j))) & ((1 << b) - 1) for j in range(n)] == vals
    n_limbs = W.n_limbs_of(n, b)
    assert n_limbs == -(-n * b // 64)
    assert np.array_equal(W.int_limbs(big, n_limbs), oracle.pack(np.array(vals, dtype=np.uint64), b))


@pytest.mark.parametrize("b", WIDTHS)
@pytest.mark.parametrize("n", LENGTHS)
def test_limb_i_of_the_byte_form_is_bits_64i_to_64i_plus_64(n, b):
    big = W.wire_int(_values(n, b), b)
    n_limbs = W.n_limbs_of(n, b)
    limbs = W.int_limbs(big, n_limbs)
    assert limbs.dtype == np.uint64 and limbs.shape == (n_limbs,)
    assert [int(w) for w in limbs] == [(big >> (64 * i)) & ((1 << 64) - 1) for i in range(n_limbs)]
    assert int.from_bytes(limbs.tobytes(), "little") == big


def test_wire_int_blocks_of_256_join_without_a_seam():
    vals = _values(3 * 256 + 1, 17)
    assert W.wire_int(vals, 17) == sum(v << (17 * (len(vals) - 1 - j)) for j, v in enumerate(vals))
    assert W.wire_int([], 17) == 0


@pytest.mark.parametrize("n,n_jobs,m", [(1, 1, 8), (5, 16, 8), (193, 193, 6), (7 * 192 + 3, 7, 6), (3 * 128 * 2, 3, 2), (1541, 3, 7), (512, 1, 8), (513, 1, 8)])
def test_tiles_follow_the_oracles_chunks(oracle, n, n_jobs, m):
    """Every element lies in exactly one tile, in order; a chunk end never lies inside a block; a tile holds 64 blocks, the last one fewer;
    ragged says that a chunk of the tile ends in a partial block."""
    bounds = oracle.chunks(n, n_jobs)
    assert bounds[0] == 0 and bounds[-1] == n
    sizes = [hi - lo for lo, hi in zip(bounds, bounds[1:])]
    tl = W.tiles(n, n_jobs, m)
    assert tl[0][0] == 0 and tl[-1][1] == n and all(a[1] == b[0] for a, b in zip(tl, tl[1:]))
    n_blocks = sum(-(-s // m) for s in sizes)
    assert len(tl) == -(-n_blocks // 64)
    for e0, e1, ragged in tl:
        inside = [(max(lo, e0), min(hi, e1)) for lo, hi in zip(bounds, bounds[1:]) if max(lo, e0) < min(hi, e1)]
        # a chunk that ends inside the tile (or with it) with a length that is no multiple of m ends in a partial block of this tile
        assert ragged == any((hi - lo_chunk) % m != 0 for lo_chunk, hi in zip(bounds, bounds[1:]) if e0 < hi <= e1 and hi > lo_chunk), (e0, e1)
        assert sum(hi - lo for lo, hi in inside) == e1 - e0
    assert [t[:2] for t in W.tiles(n, n_jobs, m) if not t[2]] == W.whole_tiles_in(n, n_jobs, m, 0, n)
