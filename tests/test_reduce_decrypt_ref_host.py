"""No GPU: tests/reduce_decrypt_ref.py against the oracle, and the shapes that tests/test_gpu_reduce_decrypt_edges.py runs against the
geometry mirror -- every shape must hold the edge its name promises, so that a GPU case cannot quietly miss it."""
import numpy as np
import pytest

import reduce_decrypt_ref as R


# ------------------------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("b", [1, 20, 32, 33, 64, 100, 128])
def test_reference_equals_the_oracles_reduce_and_combine(oracle, b):
    rng = np.random.Generator(np.random.PCG64(b))
    n, J, L = 77, 3, 2 if b > 64 else 1
    for C, with_minus in ((1, True), (3, True), (5, False), (64, True)):
        ops = [[int.from_bytes(rng.bytes(16), "little") % (1 << b) for _ in range(n)] for _ in range(C)]
        add, minus = R.mask_ints(oracle, R.ADD, n, J, b), R.mask_ints(oracle, R.MINUS, n, J, b) if with_minus else None
        agg, out = R.reference(b, ops, add, minus)
        o_agg = oracle.aggregate_elem([R.to_array(v, 16)[:, :L] for v in ops], b)
        assert R.limbs_to_ints(o_agg) == agg
        o_out = oracle.combine(b, o_agg, oracle.mask(R.KEY, R.IT, R.ADD, n, J, b), oracle.mask(R.KEY, R.IT, R.MINUS, n, J, b) if with_minus else None)
        assert R.limbs_to_ints(o_out) == out
        assert all(0 <= v < (1 << b) for v in agg + out)


def test_reference_reduces_unreduced_operands_and_wraps():
    assert R.reference(8, [[255, 256], [255, 1]], [1, 0], [0, 3]) == ([254, 1], [255, 254])
    assert R.reference(128, [[2 ** 128 - 1]] * 2, [2], None) == ([2 ** 128 - 2], [0])


# ------------------------------------------------------------------------------------------------------------------ the mirror itself
def test_chunks_and_blocks_agree_with_the_oracle_and_with_block_of(oracle):
    for n, J in ((5, 16), (1, 3), (77, 3), (1000, 7), (4097, 1), (13, 13)):
        cb = R.chunk_bounds(n, J)
        assert [s for s, _ in cb] + [n] == oracle.chunks(n, J)
        for b in (64, 33, 20, 11, 1):
            m = R.m_of(b)
            blocks = R.blocks_of_vector(n, J, m)
            assert sum(cnt for _, cnt in blocks) == n
            for j in range(n):
                j0, cnt = blocks[R.block_of(j, n, J, m)]
                assert j0 <= j < j0 + cnt, (n, J, b, j)


def test_the_e_rule():
    # as read from launch_small_reduce_decrypt: (E, active lanes of the last trip, trips of the lane loop)
    assert R.epl_of(16) == (4, 64, 1) and R.epl_of(20) == (3, 64, 1) and R.epl_of(32) == (2, 64, 1)
    assert R.epl_of(11)[0] == 2 and R.epl_of(10)[0] == 3
    assert R.epl_of(25) == (4, 40, 1)
    assert R.epl_of(1) == (4, 64, 16)
    assert set(R.epl_of(b)[0] for b in R.VECTOR_WIDTHS) == {2, 3, 4}
    assert set(R.epl_of(b)[0] for b in R.COMPACT_WIDTHS) == {2, 3, 4}


def test_the_magic_multiply_is_a_division_by_m_on_every_tile_offset():
    # the kernels take x / m as (x * ceil(2^32 / m)) >> 32 for x below the elements of a tile
    for b in R.ONE_LIMB_WIDTHS:
        m = R.m_of(b)
        magic = ((1 << 32) + m - 1) // m
        assert all((x * magic) >> 32 == x // m for x in range(R.tile_blocks(b) * m)), b
    # ... and without the rounding up it is not, at the first multiple of m already, for every m that is no power of two
    assert all((m * ((1 << 32) // m)) >> 32 != 1 for m in (3, 5, 6, 7, 9, 11, 12))


# ------------------------------------------------------------------------------------------------------------------ the shapes
@pytest.mark.parametrize("b", R.ONE_LIMB_WIDTHS)
def test_every_width_shape_has_chunk_ends_in_mid_tile_and_a_partial_last_block(b):
    n, J = R.width_shape(b)
    m, T = R.m_of(b), R.tile_blocks(b)
    f = R.features(b, n, J)
    assert f["tiles"] == 3 and f["partial_block"] and f["chunk_ends_in_a_tile"] >= 1
    blocks = R.blocks_of_vector(n, J, m)
    assert blocks[-1][1] < m                                                      # the last block is partial
    ends = [k for k, (j0, cnt) in enumerate(blocks) if j0 + cnt in set(e for _, e in R.chunk_bounds(n, J))]
    assert len(ends) == 3 and all(k % T not in (T - 1,) for k in ends[:2])        # chunk ends away from the tile's last block
    # a sub-range of it that starts and ends inside a block
    assert 0 < n // 3 + 1 < n - 2


def test_slots_straddle_words_where_the_width_says_so():
    assert [b for b in range(1, 33) if not R.straddles_a_word(b)] == [1, 2, 4, 8, 16, 32]
    assert [b for b in range(33, 65) if not R.reads_w2(b)[0]] == [64]
    # w[2] past word 3 of the lane's row (the next lane's row, the pad behind the last): wherever three slots share a block
    assert [b for b in range(33, 65) if R.reads_w2(b)[1]] == list(range(33, 43))
    assert all(R.straddles_a_word(b) for b in (20, 25, 11)) and all(R.reads_w2(b) == (True, True) for b in (33, 40))


@pytest.mark.parametrize("b", R.CHUNK_WIDTHS)
def test_chunk_shapes(b):
    m, T = R.m_of(b), R.tile_blocks(b)
    S = R.chunk_shapes(b)
    n, J = S["more_chunks_than_elements"]
    f = R.features(b, n, J)
    assert J > n and f["d"] == 0 and f["one_element_blocks"] and f["chunk_ends_in_a_tile"] == 5 >= 2 and f["tiles"] == 1
    for name, want in (("chunk_of_m", m), ("chunk_of_m_plus_1", m + 1), ("chunk_of_2m_minus_1", 2 * m - 1)):
        n, J = S[name]
        assert n // J + 1 == want and n % J >= 1, name
        assert R.features(b, n, J)["chunk_ends_in_a_tile"] == 3
    n, J = S["chunk_of_m"]
    assert [cnt for _, cnt in R.blocks_of_vector(n, J, m)] == [m, m - 1, m - 1]
    n, J = S["chunk_of_m_plus_1"]
    assert [cnt for _, cnt in R.blocks_of_vector(n, J, m)] == [m, 1, m, m]
    n, J = S["one_chunk"]
    f = R.features(b, n, J)
    assert J == 1 and f["whole_tile"] and f["partial_block"] and f["tiles"] == 2
    assert S["one_element"] == (1, 1) and S["one_element_of_three_chunks"] == (1, 3)
    assert R.features(b, 1, 3)["d"] == 0


@pytest.mark.parametrize("b", R.TRIP_WIDTHS)
def test_trip_shapes_reach_a_second_trip_of_the_one_workgroup(b):
    shapes = R.trip_shapes(b)
    tiles = [R.features(b, n, J)["tiles"] for n, J in shapes]
    # one CU: grid = 1, wave w takes tiles w, w + 16, ...: tile index 16 is the first second trip
    assert tiles[0] == 16 and tiles[1] == 16 and tiles[2] == 17 and tiles[3] == 33
    assert shapes[4][1] == 7 and tiles[4] >= 17 and R.features(b, *shapes[4])["chunk_ends_in_a_tile"] >= 1
    assert all(R.features(b, n, J)["max_tile"] >= 16 for n, J in shapes[2:])
    assert max(n for n, _ in shapes) <= 2 * 16 * 32 * 8 + 1                       # a few thousand elements


@pytest.mark.parametrize("b", R.VECTOR_WIDTHS)
def test_vector_ranges_hold_regular_tiles_inside_and_cut_at_each_end(b):
    E = R.epl_of(b)[0]
    for J in (1, 3):
        n, _ = R.vector_shape(b, J)
        ranges = R.vector_ranges(b, J)
        fs = [R.features(b, n, J, first, count) for first, count in ranges]
        assert all(first + count <= n for first, count in ranges)
        if J == 1:      # (three chunks hold two whole tiles each: the three meet in one launch only where every tile can be regular)
            assert any(f["regular_inside"] and f["cut_at_start"] and f["cut_at_end"] for f in fs), (b, J)
        assert any(f["regular_inside"] and not f["cut_at_start"] and not f["cut_at_end"] for f in fs), (b, J)
        assert any(f["cut_at_start"] for f in fs) and any(f["cut_at_end"] for f in fs) and any(f["end_one_short"] for f in fs)
        tile = 32 * R.m_of(b)
        firsts = set(first for first, _ in ranges)
        assert {0, 4, 8, tile - 4, tile, tile + 4} <= firsts
        if J == 1:
            assert all(f["partial_block"] is False or first + count == n for f, (first, count) in zip(fs, ranges))
            assert {5 * tile, 5 * tile - 4, 5 * tile - 1, 5 * tile + 1} <= set(first + count for first, count in ranges)
        else:
            starts = [s for s, _ in R.chunk_bounds(n, J)]
            assert starts[1] % 4 == 2 and starts[1] in firsts
            # a whole tile whose first element is = 0 mod 4 from `first` for no E = 4 access: declined there, taken by E = 2 and 3
            assert any(f["regular_declined_by_e4"] for f in fs), (b, J)
            if E == 4:
                t_all = [t for first, count in ranges for t in R.tiles_of_range(b, n, J, first, count)
                         if R.is_regular(t, b, first, count) and not R.is_regular(t, b, first, count, epl=4)]
                assert t_all
    if b in (25, 11):
        assert any(f["odd_e0t"] for J in (3,) for first, count in R.vector_ranges(b, J) for f in [R.features(b, R.vector_shape(b, J)[0], J, first, count)])


def test_operand_counts_cross_the_steps():
    C = R.OPERAND_COUNTS
    assert {1, 2, 3} <= set(C) and {7, 8, 9, 16, 17} <= set(C) and {63, 64} <= set(C)        # CB = 2 surplus slot; QB = 8 steps; kMaxOps
    assert {R.K_SUM_REGS - 1, R.K_SUM_REGS, R.K_SUM_REGS + 1, 1, R.MAX_OPS} == set(R.WIDE_OPERAND_COUNTS)


def test_wide_second_trip():
    assert R.wide_second_trip(1) == 1025
