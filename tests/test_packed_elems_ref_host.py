"""CPU: the reference of tests/test_gpu_packed_elems.py (tests/packed_elems_ref.py) against the oracle's pack / packed reduce / unpack and
the reference project's recorded rounds, the element-domain recurrence the kernels compute against that reference, and every named
shape against the edge it is named after."""
import numpy as np
import pytest

import packed_elems_ref as R
from conftest import load_golden, unhex


def _limbs(oracle, vals, b):
    return oracle.ints_to_limbs([v & ((1 << b) - 1) for v in vals], b).reshape(len(vals), 2 if b > 64 else 1)


@pytest.mark.parametrize("b", sorted(set(R.WIDTHS_U64 + R.WIDTHS_U32 + [1, 4, 7])))
def test_reference_is_the_oracles_pack_reduce_unpack(oracle, b):
    for n, C in ((1, 2), (65, 3), (257, min(10, 1 << b))):
        ops = R.random_ops(b, n, C)
        packed = [oracle.pack(_limbs(oracle, o, b), b) for o in ops]
        want = oracle.limbs_to_ints(oracle.unpack(oracle.aggregate_packed(packed, n * b), n, b))
        assert R.reference(b, ops) == want, (b, n, C)


def test_reference_is_the_recorded_packed_aggregate_of_the_golden_rounds():
    seen = 0
    for c in load_golden("cipher_rounds.json")["cases"]:
        b, n = c["b"], c["n"]
        if n == 0:
            continue
        ops = [unhex(c["ct"][str(i)]) for i in c["uploaded"]]
        assert sum(R.pack_int(o, b) for o in ops) % (1 << (n * b)) == int(c["agg_packed_int"], 16)
        assert R.reference(b, ops) == unhex(c["agg_packed"]), (b, n)
        if len(ops) <= (1 << b):
            assert R.recurrence(b, ops)[0] == unhex(c["agg_packed"]), (b, n)
        seen += 1
    assert seen > 0


@pytest.mark.parametrize("b", [1, 2, 3, 4, 5, 7, 8, 16, 20, 31, 32, 33, 63, 64, 65, 127, 128])
def test_recurrence_is_the_reference(b):
    """Random operands, operands of long all-ones runs, every operand count up to 2^b (at most 64) at small widths."""
    rng = np.random.Generator(np.random.PCG64(b))
    M = (1 << b) - 1
    counts = sorted(set(c for c in (1, 2, 3, 10, 16, 17, 63, 64) if c <= (1 << b)) | {min(64, 1 << b)})
    for C in counts:
        for n in (1, 2, 7, 70):
            ops = R.random_ops(b, n, C, seed=C)
            assert R.recurrence(b, ops)[0] == R.reference(b, ops), (b, C, n)
            runs = [[M if rng.random() < 0.8 else int(rng.integers(0, 4)) for _ in range(n)] for _ in range(C)]
            assert R.recurrence(b, runs)[0] == R.reference(b, runs), (b, C, n)
            assert R.recurrence(b, R.all_ones(b, n, C))[0] == R.reference(b, R.all_ones(b, n, C))


def test_one_operand_more_than_two_to_the_width_needs_a_wider_carry():
    """b = 4, C = 17: the column sums' high part reaches 16 > M, which the one-bit chain cannot hold -- the entry point's ENOTSUP rule."""
    ops = R.all_ones(4, 3, 17)
    with pytest.raises(AssertionError):
        R.recurrence(4, ops)
    assert R.recurrence(4, R.all_ones(4, 3, 16))[0] == R.reference(4, R.all_ones(4, 3, 16))


@pytest.mark.parametrize("b", [8, 20, 64, 122, 128])
def test_named_shapes_hold_their_edges(b):
    n, M = R.N_PATTERN, (1 << b) - 1
    nb = -(-n // R.TILE)
    assert nb == 6 and n % R.TILE == 3 and R.STOP_RANK // R.TILE == 2
    assert set(R.LENGTHS) >= {1, 2, R.WAVE - 1, R.WAVE, R.WAVE + 1, R.TILE - 1, R.TILE, R.TILE + 1, 2 * R.TILE + 1, n}
    # random over the container: some bit above b is set wherever the container is wider than b
    for compact in ([False, True] if b <= 32 else [False]):
        ops = R.random_ops(b, n, 10, compact)
        if 8 * R.elem_bytes(b, compact) > b:
            assert any(v >> b for o in ops for v in o)
        out, h, g, p = R.recurrence(b, ops)
        assert out == R.reference(b, ops)
        # ... and most elements differ from the element-wise sum by what their neighbour's column carries in
        elem = [sum(o[j] for o in ops) & M for j in range(n)]
        assert sum(x != y for x, y in zip(out, elem)) > n // 4
    # all ones: h = C - 1 in every column
    out, h, g, p = R.recurrence(b, R.all_ones(b, n, 10))
    assert set(h) == {9} and out == R.reference(b, R.all_ones(b, n, 10))
    # ripple-out: every block but the first fully propagates, the first generates; all zeros
    out, h, g, p = R.recurrence(b, R.ripple_out(b, n))
    assert out == [0] * n == R.reference(b, R.ripple_out(b, n))
    assert R.block_summaries(g, p) == [(1, 0)] + [(0, 1)] * (nb - 1)
    # ripple-stop: block 2's carry-in is block 0's generate seen through the fully propagating block 1; block 2 absorbs it
    out, h, g, p = R.recurrence(b, R.ripple_stop(b, n))
    assert R.block_summaries(g, p) == [(1, 0), (0, 1), (0, 0)] + [(0, 1)] * (nb - 3)
    assert R.by_rank(n, out) == [0] * R.STOP_RANK + [M] * (n - R.STOP_RANK) and out == R.reference(b, R.ripple_stop(b, n))
    # the chains end exactly one element past a wave edge / a block edge
    for end in (R.WAVE, R.TILE):
        out, h, g, p = R.recurrence(b, R.chain_to(b, n, end))
        assert R.by_rank(n, out) == [0] * end + [6] + [5] * (n - end - 1) and out == R.reference(b, R.chain_to(b, n, end))
    assert set(R.patterns(b)) == {"random", "all-ones", "ripple-out", "ripple-stop", "chain-past-wave", "chain-past-block"}


@pytest.mark.parametrize("b", [16, 20, 32])
def test_named_shapes_hold_the_vector_kernels_edges(b):
    """Four elements per lane: blocks of 1024 ranks and waves of 256, counted from the padded length (one virtual element here)."""
    n, M = R.N_PATTERN_X4, (1 << b) - 1
    pad = R.pad_x4(n)
    nb = -(-(n + pad) // R.TILE_X4)
    assert pad == 1 and nb == 6 and [R.pad_x4(k) for k in (4, 5, 6, 7)] == [0, 3, 2, 1]
    assert set(R.LENGTHS_X4) >= {1, 2, 3, 4, 5, R.WAVE_X4 - 1, R.WAVE_X4, R.WAVE_X4 + 1, R.TILE_X4 - 1, R.TILE_X4, R.TILE_X4 + 1, 2 * R.TILE_X4 + 1, n}
    pats = R.patterns(b, n, compact=True, x4=True)
    for name, ops in pats.items():
        assert R.recurrence(b, ops)[0] == R.reference(b, ops), name
    out, h, g, p = R.recurrence(b, pats["ripple-out"])
    assert out == [0] * n and R.block_summaries(g, p, R.TILE_X4, pad) == [(1, 0)] + [(0, 1)] * (nb - 1)
    out, h, g, p = R.recurrence(b, pats["ripple-stop"])
    assert R.block_summaries(g, p, R.TILE_X4, pad) == [(1, 0), (0, 1), (0, 0)] + [(0, 1)] * (nb - 3)
    for name, edge in (("chain-past-wave", R.WAVE_X4), ("chain-past-block", R.TILE_X4)):
        out = R.by_rank(n, R.recurrence(b, pats[name])[0])
        assert out == [0] * (edge - pad) + [6] + [5] * (n - edge + pad - 1)        # absorbed at padded rank `edge`: one past the edge
