"""GPU: the arbiter's reduce fused with the decrypt of its result at tile, chunk and width edges --

    small_reduce_decrypt_kernel<CB, 2>                (33 <= int_bits <= 64: tiles of 64 AES blocks)
    small_reduce_decrypt_split_kernel<CB, IT, OT>     (int_bits <= 32: tiles of 32 blocks; u64 -> u64, u32 -> u64, u32 -> u32 and the
                                                       u32 -> u32 vector path of E = 2, 3 or 4 elements per lane)
    reduce_decrypt_ptrs_kernel<DBL>                   (int_bits > 64: a grid-stride loop over a pointer table)
    the C = 1 shortcut of flashe_aggregate_decrypt_u32_dev (launch_prf_chains)

through Engine.aggregate_decrypt_range_dev and Engine.aggregate_decrypt_u32_dev.  Every value is compared exactly with
tests/reduce_decrypt_ref.py (Python integers, the oracle's masks); operands and outputs lie between guard zones in one poisoned block
that is read back whole, so a store outside an output or into an operand fails the case.  The shapes come from reduce_decrypt_ref.py,
where tests/test_reduce_decrypt_ref_host.py asserts without a GPU that each one holds the edge it is named after.  Operands are
random over the whole element (not reduced mod 2^b) unless the case sets them."""
import numpy as np
import pytest

import reduce_decrypt_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    from flashe_amd import engine
    return engine


@pytest.fixture(scope="module")
def engines(E):
    """One engine per width (and one more per width on ONE compute unit) for the groups whose widths are fixed."""
    cache = {}

    def get(b, one_cu=False):
        if (b, one_cu) not in cache:
            e = E.Engine(R.KEY, b, device=0)
            if one_cu:
                e.set_cu_limit(1)
            cache[b, one_cu] = e
        return cache[b, one_cu]

    yield get
    for e in cache.values():
        e.close()


class Vec:
    """C operands of an n-vector in J chunks as bytes (what is uploaded) and as Python ints, with the reference computed ONCE; a launch
    on a sub-range compares with a slice of it.  in_elem: bytes per operand element (4: the compact layout, 8, 16)."""

    def __init__(self, oracle, b, n, J, C, in_elem, ops=None, seed=0):
        self.b, self.n, self.J, self.C, self.in_elem = b, n, J, C, in_elem
        if ops is None:
            rng = np.random.Generator(np.random.PCG64([b, n, J, C, in_elem, seed]))
            self.arrs = [np.frombuffer(rng.bytes(n * in_elem), dtype=np.uint8) for _ in range(C)]
        else:
            self.arrs = [R.to_array(v, in_elem).view(np.uint8).reshape(-1) for v in ops]
        ints = []
        for a in self.arrs:
            if in_elem == 4:
                ints.append(a.view(np.uint32).tolist())
            else:
                w = a.view(np.uint64).tolist()
                ints.append(w if in_elem == 8 else [lo | (hi << 64) for lo, hi in zip(w[0::2], w[1::2])])
        add, minus = R.mask_ints(oracle, R.ADD, n, J, b), R.mask_ints(oracle, R.MINUS, n, J, b)
        self.agg, self.out = R.reference(b, ints, add, minus)
        _, self.out_no_minus = R.reference(b, ints, add, None)


def _same(got, want, ctx):
    if got != want:
        bad = [k for k, (g, w) in enumerate(zip(got, want)) if g != w]
        pytest.fail("%r: %d of %d elements differ, the first at %d: got %#x, want %#x" % (ctx, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]]))


def launch(eng, v, out_elem=None, first=0, count=None, minus=True, agg=True, shift=None, separate=False, refused=False):
    """One call on [first, first + count) (pointers address element `first`), compared with the reference.  shift: {"out" | "agg" |
    "op<c>": bytes past a 16-byte boundary}; separate: every operand in an allocation of its own instead of equally spaced in the block."""
    count = v.n - first if count is None else count
    ie = v.in_elem
    oe = ie if out_elem is None else out_elem
    shift = shift or {}
    ctx = dict(b=v.b, n=v.n, J=v.J, C=v.C, elems=(ie, oe), first=first, count=count, minus=minus, agg=agg, shift=shift, separate=separate)
    a, held, ptrs = R.Arena(eng), [], []
    try:
        for c in range(v.C):
            data = v.arrs[c][first * ie:(first + count) * ie]
            if separate:
                held.append(eng.upload(data))
            else:
                a.add("op%d" % c, data.nbytes, data, shift.get("op%d" % c, 0))
        if agg:
            a.add("agg", count * oe, None, shift.get("agg", 0))
        a.add("out", count * oe, None, shift.get("out", 0))
        a.commit()
        ptrs = [h.ptr for h in held] if separate else [a.ptr("op%d" % c) for c in range(v.C)]
        args = (R.IT, [R.ADD], [R.MINUS] if minus else [], v.n, v.J, first, count, ptrs, a.ptr("agg") if agg else None, a.ptr("out"))
        call = (lambda: eng.aggregate_decrypt_u32_dev(*args, out_elem_bytes=oe)) if ie == 4 else (lambda: eng.aggregate_decrypt_range_dev(*args))
        if refused:
            from flashe_amd._lib import FlasheError
            with pytest.raises(FlasheError):
                call()
            eng.sync()
            a.fetch()
            assert a.untouched("out") and (not agg or a.untouched("agg")), ctx
            return
        call()
        a.fetch()
        if agg:
            _same(a.values("agg", oe), v.agg[first:first + count], ("agg", ctx))
        _same(a.values("out", oe), (v.out if minus else v.out_no_minus)[first:first + count], ("out", ctx))
    finally:
        a.free()
        for h in held:
            h.free()


def forms(b):
    """(operand element bytes, output element bytes) of every layout a width has: one limb (two above 64 bits), compact -> u32, compact -> u64"""
    if b > 64:
        return [(16, 16)]
    return [(8, 8)] + ([(4, 4), (4, 8)] if b <= 32 else [])


# ------------------------------------------------------------------------------------------------------------------ 1. every width
@pytest.mark.parametrize("b", R.ONE_LIMB_WIDTHS)
def test_every_width_in_every_layout(E, oracle, b):
    """n = (2 T + 5) m + 3 in three chunks: chunk ends in mid tile, the last block partial, three tiles; C = 3.  With and without a minus
    prefix (the split kernel's upper half-wave must then contribute zeros), with and without agg_out, the whole vector and a range that
    starts and ends inside a block."""
    eng = E.Engine(R.KEY, b, device=0)
    try:
        n, J = R.width_shape(b)
        f0, cnt = n // 3 + 1, n - n // 3 - 3
        for ie in sorted(set(ie for ie, _ in forms(b))):
            v = Vec(oracle, b, n, J, 3, ie)
            for oe in [o for i, o in forms(b) if i == ie]:
                launch(eng, v, oe, agg=True)
                launch(eng, v, oe, minus=False, agg=False)
                launch(eng, v, oe, f0, cnt, agg=False)
                launch(eng, v, oe, f0, cnt, minus=False, agg=True)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------ 2. chunks
@pytest.mark.parametrize("b", R.CHUNK_WIDTHS)
def test_chunk_lengths_around_a_block(engines, oracle, b):
    eng = engines(b)
    for name, (n, J) in R.chunk_shapes(b).items():
        for ie in sorted(set(ie for ie, _ in forms(b))):
            v = Vec(oracle, b, n, J, 3, ie)
            for k, oe in enumerate(o for i, o in forms(b) if i == ie):
                launch(eng, v, oe, agg=k == 0)
                launch(eng, v, oe, minus=False, agg=k != 0)
                if n > 2:
                    launch(eng, v, oe, 1, n - 2, agg=True)


# ------------------------------------------------------------------------------------------------------------------ 3. trips
@pytest.mark.parametrize("b", R.TRIP_WIDTHS)
def test_a_waves_second_trip_on_one_compute_unit(engines, oracle, b):
    """grid = min(groups of 16 tiles, compute units) = 1: tile 16 is wave 0's second trip."""
    eng = engines(b, one_cu=True)
    for n, J in R.trip_shapes(b):
        for ie in sorted(set(ie for ie, _ in forms(b))):
            v = Vec(oracle, b, n, J, 2, ie)
            for k, oe in enumerate(o for i, o in forms(b) if i == ie):
                launch(eng, v, oe, agg=k == 0)
                launch(eng, v, oe, n // 2 + 1, n - n // 2 - 1, minus=False, agg=k != 0)


# ------------------------------------------------------------------------------------------------------------------ 4. the vector path
@pytest.mark.parametrize("J", [1, 3])
@pytest.mark.parametrize("b", R.VECTOR_WIDTHS)
def test_compact_vector_path_on_sub_ranges(engines, oracle, b, J):
    """16-byte aligned pointers (they address element `first`): regular tiles take E = 2, 3 or 4 elements per lane and access.  Ranges
    that start and end inside a tile, on its boundary and inside its first / last block; J = 3: a chunk that starts at an element
    = 2 mod 4, so that E = 4 must decline its tiles.  Then one pointer 4 or 8 bytes off: the path must switch itself off."""
    eng = engines(b)
    n, _ = R.vector_shape(b, J)
    v = Vec(oracle, b, n, J, 3, 4)
    for i, (first, count) in enumerate(R.vector_ranges(b, J)):
        launch(eng, v, 4, first, count, agg=True)
        launch(eng, v, 4, first, count, agg=False, minus=bool(i & 1))
        s1, s2 = (4, 8) if i & 1 else (8, 4)
        launch(eng, v, 4, first, count, agg=True, shift={"out": s1})
        launch(eng, v, 4, first, count, agg=True, shift={"agg": s2})
        launch(eng, v, 4, first, count, agg=bool(i & 2), shift={"op%d" % (i % 3): s1})


# ------------------------------------------------------------------------------------------------------------------ 5. operand counts
@pytest.mark.parametrize("C", R.OPERAND_COUNTS)
def test_operand_counts_of_the_small_kernels(engines, oracle, C):
    """b = 20 compact and aligned: the vector path's steps of QB = 8 operands; b = 20 and b = 40 in the one-limb layout: steps of CB = 2,
    whose surplus slot re-reads operand C - 1 and must not add it.  Operands in allocations of their own, and equally spaced in one."""
    n, J = R.vector_shape(20, 1)
    v = Vec(oracle, 20, n, J, C, 4)
    for separate in (True, False):
        launch(engines(20), v, 4, agg=separate, separate=separate)
        launch(engines(20), v, 4, 4, n - 9, agg=not separate, minus=False, separate=separate)
        launch(engines(20), v, 8, agg=separate, separate=separate)
    for b in (20, 40):
        n, J = R.width_shape(b)
        v = Vec(oracle, b, n, J, C, 8)
        for separate in (True, False):
            launch(engines(b), v, agg=separate, separate=separate)
            launch(engines(b), v, first=3, count=n - 4, agg=not separate, minus=False, separate=separate)


@pytest.mark.parametrize("C", R.WIDE_OPERAND_COUNTS)
@pytest.mark.parametrize("b", [128, 100])
def test_operand_counts_of_the_wide_kernel(engines, oracle, b, C):
    """kSumRegs = 10 operands are held in registers across the rounds, the rest is summed up front."""
    n, J = 1300, 3
    v = Vec(oracle, b, n, J, C, 16)
    for separate in (True, False):
        launch(engines(b), v, agg=separate, separate=separate)
        launch(engines(b), v, first=7, count=n - 8, agg=not separate, minus=False, separate=separate)


def test_one_operand_more_than_a_launch_takes(engines, oracle):
    """C = 65: the one-limb and the wide forms fall back to two launches; the compact form refuses and writes nothing."""
    C = R.MAX_OPS + 1
    for b in (20, 40, 128, 100):
        n, J = (R.width_shape(b) if b <= 64 else (300, 3))
        v = Vec(oracle, b, n, J, C, 8 if b <= 64 else 16)
        launch(engines(b), v, agg=True)
        launch(engines(b), v, first=3, count=n - 4, agg=False)
        launch(engines(b), v, agg=False, minus=False, separate=True)
    n, J = R.width_shape(20)
    v = Vec(oracle, 20, n, J, C, 4)
    for oe in (4, 8):
        launch(engines(20), v, oe, agg=True, refused=True)
        launch(engines(20), v, oe, first=3, count=n - 4, agg=False, refused=True)


# ------------------------------------------------------------------------------------------------------------------ 6. wrap
@pytest.mark.parametrize("C", [64, 2])
@pytest.mark.parametrize("b", R.WRAP_SMALL + R.WRAP_WIDE)
def test_sums_that_wrap(engines, oracle, b, C):
    """Every operand 2^b - 1 (b > 64: low limbs all ones -- the carry into the high limb -- and high limbs 2^(b - 64) - 1), and every
    operand all ones over its whole element: the 32-, 64- and 128-bit accumulators wrap."""
    n, J = R.width_shape(b) if b <= 64 else (1300, 3)
    for ie in sorted(set(ie for ie, _ in forms(b))):
        for top in ((1 << b) - 1, (1 << (8 * ie)) - 1):
            v = Vec(oracle, b, n, J, C, ie, ops=[[top] * n] * C)
            assert v.agg[0] == (C * top) % (1 << b)
            for k, oe in enumerate(o for i, o in forms(b) if i == ie):
                launch(engines(b), v, oe, agg=True)
                launch(engines(b), v, oe, 5, n - 6, agg=False, minus=bool(k))


# ------------------------------------------------------------------------------------------------------------------ 7. C = 1
@pytest.mark.parametrize("J", [1, 3])
@pytest.mark.parametrize("b", [20, 32])
def test_one_operand_by_the_chain_shortcut_and_by_the_reduce_kernel(engines, oracle, b, J):
    """No agg_out, a 4-byte out and a minus prefix: launch_prf_chains; agg_out given: the reduce kernel.  The same sub-ranges, both
    against the reference."""
    eng = engines(b)
    n, _ = R.vector_shape(b, J)
    v = Vec(oracle, b, n, J, 1, 4)
    for first, count in R.vector_ranges(b, J):
        launch(eng, v, 4, first, count, agg=False)          # the shortcut
        launch(eng, v, 4, first, count, agg=True)           # the reduce kernel
    launch(eng, v, 4, agg=False, minus=False)               # (no minus prefix: the reduce kernel again)
    launch(eng, v, 8, agg=False)                            # (an 8-byte out: the reduce kernel again)
    launch(eng, v, 4, agg=False, shift={"out": 4})          # the shortcut into an out that is only 4-byte aligned
    launch(eng, v, 4, 1, n - 2, agg=False, shift={"op0": 8})


# ------------------------------------------------------------------------------------------------------------------ 8. the wide range
@pytest.mark.parametrize("b", R.WIDE_WIDTHS)
def test_wide_kernels_second_trip_and_its_fallback(engines, oracle, b):
    """One compute unit: grid = grid_for(count, 1024) = 1, so a lane makes its second trip from count = 1025 on.  first is odd; once the
    range ends the vector.  An operand 8 bytes off alignment takes the two-launch fallback and must give the same answer."""
    eng = engines(b, one_cu=True)
    c2 = R.wide_second_trip(1)
    first = 7
    n = first + c2 + 1
    v = Vec(oracle, b, n, 3, 3, 16)
    for count in (c2 - 1, c2, c2 + 1):
        launch(eng, v, None, first, count, agg=True)
        launch(eng, v, None, first, count, agg=False, minus=False)
        launch(eng, v, None, first, count, agg=count != c2, shift={"op%d" % (count % 3): 8})
    assert first + c2 + 1 == n
    # the fallback's reduce on its own: flashe_aggregate_elem_dev with a two-limb operand 8 bytes off (one element per lane, 8-byte loads)
    for count, off in ((1, 0), (257, 1), (n, 2)):
        a = R.Arena(eng)
        for c in range(3):
            a.add("op%d" % c, 16 * count, v.arrs[c][:16 * count], 8 if c == off else 0)
        a.add("out", 16 * count).commit()
        try:
            eng.aggregate_elem_dev([a.ptr("op%d" % c) for c in range(3)], count, a.ptr("out"))
            _same(a.fetch().values("out", 16), v.agg[:count], ("aggregate_elem_dev", b, count, off))
        finally:
            a.free()
