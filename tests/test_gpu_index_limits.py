"""The PRF kernels at their 32-bit limits, element by element against the plain model of tests/elementwise_ref.py.

Every kernel switches between 32-bit and 64-bit index arithmetic somewhere: int_bits <= 64 takes 32-bit chunk arithmetic below
n = 2^32 (small_block_params, udiv_magic, the chained and reduce-decrypt launches) and 64-bit divisions with a non-zero high counter
word above it (prf_small_jobs_kernel, prf_small_kernel); the summed chains fold first >> 32 into their prefix words; the int_bits =
128 summed kernel addresses through 32-bit buffer offsets up to kSum128MaxCount elements; the sparse passes take uint32 positions.
The range entry points take pointers that address element `first` while n describes the whole vector, so a test can declare
n = 2^40 and allocate only the window it checks.

Every output is poisoned first and read back with the guard bytes on both sides of the range that was written."""
import numpy as np
import pytest

import elementwise_ref as ref

pytestmark = pytest.mark.gpu

KEY = bytes(range(32))
POISON = 0xC7
GUARD = 4096


@pytest.fixture(scope="module")
def E():
    from flashe_amd import engine
    return engine


def L(b):
    return 2 if b > 64 else 1


class Slab:
    """k vectors of `count` elements of `elem` bytes, each between guard zones, in one poisoned block: vector v starts at
    ptr(v), the vectors are equally spaced (the one-pass aggregate wants that)."""

    def __init__(self, eng, count, elem, k=1, guard=GUARD):
        self.count, self.elem, self.k, self.guard = count, elem, k, guard
        self.stride = count * elem + guard
        self.buf = eng.alloc(guard + k * self.stride)
        eng.memset_dev(self.buf, POISON, self.buf.nbytes)

    def ptr(self, v=0):
        return self.buf.ptr + self.guard + v * self.stride

    def check_guards(self):
        for v in range(self.k):
            for off in (v * self.stride, self.guard + v * self.stride + self.count * self.elem):
                g = self.buf.download_at(off, np.uint8, self.guard)
                assert (g == POISON).all(), ("guard bytes overwritten", v, off)

    def values(self, v=0, k0=0, k1=None):
        """Elements [k0, k1) of vector v as Python ints."""
        k1 = self.count if k1 is None else k1
        off = self.guard + v * self.stride + k0 * self.elem
        if self.elem == 4:
            return [int(x) for x in self.buf.download_at(off, np.uint32, k1 - k0)]
        raw = self.buf.download_at(off, np.uint64, (k1 - k0) * self.elem // 8).reshape(k1 - k0, self.elem // 8)
        if self.elem == 8:
            return [int(x) for x in raw[:, 0]]
        return [int(lo) | (int(hi) << 64) for lo, hi in zip(raw[:, 0], raw[:, 1])]

    def all_values(self, v=0):
        self.check_guards()
        return self.values(v)

    def free(self):
        self.buf.free()


def _rand_u64(rng, count):
    return rng.integers(0, 2 ** 64, count, dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------------------- A. one limb
IT = 13
# every width, every n and every n_jobs of the issue at least once; n >= 2^32 with a counter high word (a chunk beginning above 2^32
# or m * 2^32 < n in one chunk) at several widths
A_CONFIGS = [
    (1, 2 ** 32 - 1, 1), (7, 2 ** 32, 3), (16, 2 ** 32 + 1, 16), (20, 3 * 2 ** 32 + 12345, 17), (23, 2 ** 40 + 3, 1),
    (24, 2 ** 32 - 1, 3), (32, 2 ** 32 - 1, 16), (33, 2 ** 32 + 1, 17), (48, 3 * 2 ** 32 + 12345, 1), (63, 2 ** 40 + 3, 3),
    (64, 2 ** 32 - 1, 17), (64, 2 ** 40 + 3, 1), (20, 2 ** 32 - 1, 17), (32, 2 ** 32, 1), (7, 2 ** 40 + 3, 16),
]


def a_windows(n, J, m, w=1201):
    """(first, count) windows of w elements (odd, so that both ends fall mid-block) around: element 0; the first chunk that begins
    at or above 2^32; the first d-element chunk; the last chunk; the block whose counter begin + i is 2^32 inside a chunk; the tail."""
    ch = ref.chunk_bounds(n, J)
    d, r = divmod(n, J)
    marks = set()
    for s, e in ch:
        if s >= 2 ** 32:
            marks.add(s)
            break
    if 0 < r < J:
        marks.add(r * (d + 1))
    if J > 1:
        marks.add(ch[-1][0])
    for s, e in ch:
        if s < 2 ** 32 and s + (e - s + m - 1) // m > 2 ** 32:
            marks.add(s + (2 ** 32 - s) * m)
    out = [(0, w)]
    for p in sorted(marks):
        lo = min(max(0, p - w // 2), n - w)
        out.append((lo, w))
    out.append((n - (w - 4), w - 4))
    return sorted(set(out))


def _modsum(b, *cols):
    return [sum(v) % (1 << b) for v in zip(*cols)]


@pytest.mark.parametrize("b, n, J", A_CONFIGS)
def test_one_limb_across_2_32(E, b, n, J):
    eng = E.Engine(KEY, b, device=0)
    rng = np.random.Generator(np.random.PCG64(b * 1000 + J + n % 997))
    for first, count in a_windows(n, J, 128 // b):
        js = range(first, first + count)
        T = {i: [ref.term(KEY, IT, i, n, J, b, j) for j in js] for i in (0, 3, 4, 5, 6, 7, 8, 9, 12)}
        neg = lambda col: [-t for t in col]
        ctx = (b, n, J, first, count)

        # mask_range_dev: one prefix (job-table / chained kernel), three prefixes (prf_small_kernel)
        for lst in ([3], [3, 7, 12]):
            out = Slab(eng, count, 8)
            eng.mask_range_dev(IT, lst, n, J, first, count, out.ptr())
            assert out.all_values() == _modsum(b, *[T[i] for i in lst]), ctx + ("mask", lst)

        # encrypt_range_dev, single and double, unreduced uint64 plaintexts
        pt = _rand_u64(rng, count)
        d_pt = eng.upload(pt)
        ptl = [int(v) for v in pt]
        for scheme, want in ((E.SCHEME_SINGLE, _modsum(b, ptl, T[5])), (E.SCHEME_DOUBLE, _modsum(b, ptl, T[5], neg(T[6])))):
            out = Slab(eng, count, 8)
            eng.encrypt_range_dev(IT, 5, scheme, n, J, first, count, d_pt, 1, out.ptr())
            assert out.all_values() == want, ctx + ("encrypt", scheme)

        # decrypt_range_dev: one add / one minus prefix, and the dropout lists of two runs
        x = _rand_u64(rng, count)
        d_x = eng.upload(x)
        xl = [int(v) for v in x]
        for add, minus in (([6], [3]), ([4, 9], [0, 7])):
            out = Slab(eng, count, 8)
            eng.decrypt_range_dev(IT, add, minus, n, J, first, count, d_x, out.ptr())
            want = _modsum(b, xl, *[T[i] for i in add], *[neg(T[i]) for i in minus])
            assert out.all_values() == want, ctx + ("decrypt", add, minus)

        # prf_jobs_dev: three entries on different sub-ranges, with and without an input
        cuts = [0, count // 3 + 1, 2 * count // 3, count]
        outs = [Slab(eng, cuts[e + 1] - cuts[e], 8) for e in range(3)]
        pairs = [(4, 3), (9, 0), (12, 7)]
        jobs = []
        for e, (a, mi) in enumerate(pairs):
            inp = None if e == 1 else d_x.ptr + 8 * cuts[e]
            jobs.append((a, mi, first + cuts[e], cuts[e + 1] - cuts[e], inp, 1, outs[e].ptr()))
        eng.prf_jobs_dev(IT, n, J, jobs)
        for e, (a, mi) in enumerate(pairs):
            k0, k1 = cuts[e], cuts[e + 1]
            base = [0] * (k1 - k0) if e == 1 else xl[k0:k1]
            assert outs[e].all_values() == _modsum(b, base, T[a][k0:k1], neg(T[mi][k0:k1])), ctx + ("jobs", e)

        # encrypt_batch_range_dev with the sum: a run of consecutive clients, and a broken run
        pts = [_rand_u64(rng, count) for _ in range(3)]
        d_pts = [eng.upload(p) for p in pts]
        ptls = [[int(v) for v in p] for p in pts]
        for idx in ([3, 4, 5], [3, 4, 7]):
            cts, sm = Slab(eng, count, 8, k=3), Slab(eng, count, 8)
            eng.encrypt_batch_range_dev(IT, idx, E.SCHEME_DOUBLE, n, J, first, count, d_pts, 1, [cts.ptr(v) for v in range(3)], sm.ptr())
            cts.check_guards()
            want_ct = [_modsum(b, ptls[v], T[i], neg(T[i + 1])) for v, i in enumerate(idx)]
            for v in range(3):
                assert cts.values(v) == want_ct[v], ctx + ("batch ciphertext", idx, v)
            assert sm.all_values() == _modsum(b, *want_ct), ctx + ("batch sum", idx)

        # aggregate_decrypt_range_dev, C = 3 (the last batch's ciphertexts, equally spaced)
        agg, out = Slab(eng, count, 8), Slab(eng, count, 8)
        eng.aggregate_decrypt_range_dev(IT, [6], [3], n, J, first, count, [cts.ptr(v) for v in range(3)], agg.ptr(), out.ptr())
        want_agg = _modsum(b, *want_ct)
        assert agg.all_values() == want_agg, ctx + ("aggregate",)
        assert out.all_values() == _modsum(b, want_agg, T[6], neg(T[3])), ctx + ("aggregate decrypt",)

        # the compact layout's aggregate decrypt (b <= 32, n < 2^32)
        if b <= 32 and n < 2 ** 32 and eng.compact_supported():
            c32 = Slab(eng, count, 4, k=3)
            vals = [rng.integers(0, 1 << b, count, dtype=np.uint64).astype(np.uint32) for _ in range(3)]
            for v in range(3):
                c32.buf.upload_at(c32.guard + v * c32.stride, vals[v])
            want_agg = _modsum(b, *[[int(t) for t in v] for v in vals])
            for elem in (4, 8):                 # agg_out and out are both uint32 or both uint64
                agg, out = Slab(eng, count, elem), Slab(eng, count, elem)
                eng.aggregate_decrypt_u32_dev(IT, [6], [3], n, J, first, count, [c32.ptr(v) for v in range(3)], agg.ptr(), out.ptr(), elem)
                assert agg.all_values() == want_agg, ctx + ("u32 aggregate", elem)
                assert out.all_values() == _modsum(b, want_agg, T[6], neg(T[3])), ctx + ("u32 aggregate decrypt", elem)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- B. wide summed chains
def _sum_u64_exact(pts):
    """sum of one-limb vectors as (lo, hi) uint64 arrays, exactly (no wrap below 2^128)."""
    lo = np.zeros_like(pts[0])
    hi = np.zeros_like(pts[0])
    for p in pts:
        s = lo + p
        hi += (s < lo).astype(np.uint64)
        lo = s
    return lo, hi


def _sum_limbs(vecs, b):
    """sum of two-limb vectors [count, 2] mod 2^b as [count, 2]."""
    lo = np.zeros(vecs[0].shape[0], dtype=np.uint64)
    hi = np.zeros_like(lo)
    for v in vecs:
        s = lo + v[:, 0]
        hi = hi + v[:, 1] + (s < lo).astype(np.uint64)
        lo = s
    if b < 128:
        hi &= np.uint64((1 << (b - 64)) - 1)
    return np.stack([lo, hi], axis=1)


SUMMED_MIN = 2_097_152          # launch_prf_batch_sum: two 256-element tiles per wave of 256 CUs x 16 waves


@pytest.mark.parametrize("b", [128, 100])
@pytest.mark.parametrize("first, count", [(2 ** 32 + 256 * 4001 + 77, SUMMED_MIN + 2_851),      # above 2^32, starting mid-tile
                                          (2 ** 32 - 1_000_003, SUMMED_MIN + 3_000)])           # straddling 2^32: the fallback
def test_summed_chain_beyond_2_32(E, b, first, count):
    eng = E.Engine(KEY, b, device=0)
    n, J, it, idx = 2 ** 34 + 5, 16, 21, [4, 5, 6]
    rng = np.random.Generator(np.random.PCG64(first % 100_003 + b))
    pts = [_rand_u64(rng, count) for _ in idx]
    d_pts = [eng.upload(p) for p in pts]
    cts, sm = Slab(eng, count, 16, k=3), Slab(eng, count, 16)
    eng.encrypt_batch_range_dev(it, idx, E.SCHEME_DOUBLE, n, J, first, count, d_pts, 1, [cts.ptr(v) for v in range(3)], sm.ptr())
    cts.check_guards()
    sm.check_guards()
    got_ct = [cts.buf.download_at(cts.guard + v * cts.stride, np.uint64, 2 * count).reshape(count, 2) for v in range(3)]
    got_sum = sm.buf.download_at(sm.guard, np.uint64, 2 * count).reshape(count, 2)
    assert np.array_equal(got_sum, _sum_limbs(got_ct, b)), "sum != sum of the ciphertexts"

    # the model on windows: both ends, the middle, and the element whose counter is 2^32 when the range straddles it
    wins = [(0, 600), (count // 2 - 301, 600), (count - 600, 600)]
    if first < 2 ** 32 < first + count:
        wins.append((2 ** 32 - first - 300, 600))
    for k0, w in wins:
        js = range(first + k0, first + k0 + w)
        T = {i: [ref.term(KEY, it, i, n, J, b, j) for j in js] for i in (4, 5, 6, 7)}
        for v, i in enumerate(idx):
            want = [(int(pts[v][k0 + k]) + T[i][k] - T[i + 1][k]) % (1 << b) for k in range(w)]
            got = [int(lo) | (int(hi) << 64) for lo, hi in got_ct[v][k0:k0 + w]]
            assert got == want, (b, first, count, "ciphertext", v, k0)

    # the decrypt with the chain's (add, minus): through D where the launch wrote it, by the PRF otherwise -- the plaintexts' sum
    lo, hi = _sum_u64_exact(pts)
    out = Slab(eng, count, 16)
    eng.decrypt_range_dev(it, [idx[-1] + 1], [idx[0]], n, J, first, count, sm.ptr(), out.ptr())
    out.check_guards()
    got = out.buf.download_at(out.guard, np.uint64, 2 * count).reshape(count, 2)
    assert np.array_equal(got[:, 0], lo) and np.array_equal(got[:, 1], hi), (b, first, count, "decrypt")
    # ... and on a window inside, against the model
    k0, w = count // 3, 777
    sub = Slab(eng, w, 16)
    eng.decrypt_range_dev(it, [idx[-1] + 1], [idx[0]], n, J, first + k0, w, sm.ptr() + 16 * k0, sub.ptr())
    sums = [int(a) | (int(c) << 64) for a, c in got_sum[k0:k0 + w]]
    assert sub.all_values() == ref.decrypt(KEY, it, [7], [4], n, J, b, range(first + k0, first + k0 + w), sums), (b, first, "sub-range decrypt")

    # the one-pass aggregate decrypt of the same (equally spaced) ciphertexts
    agg, out2 = Slab(eng, count, 16), Slab(eng, count, 16)
    eng.aggregate_decrypt_range_dev(it, [idx[-1] + 1], [idx[0]], n, J, first, count, [cts.ptr(v) for v in range(3)], agg.ptr(), out2.ptr())
    agg.check_guards()
    out2.check_guards()
    assert np.array_equal(agg.buf.download_at(agg.guard, np.uint64, 2 * count).reshape(count, 2), got_sum), (b, first, "aggregate")
    got2 = out2.buf.download_at(out2.guard, np.uint64, 2 * count).reshape(count, 2)
    assert np.array_equal(got2[:, 0], lo) and np.array_equal(got2[:, 1], hi), (b, first, "aggregate decrypt")
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- C. the 4 GiB edge
SUM128_MAX = 0x0fffff00         # kSum128MaxCount: the largest count prf_dmask_sum128_kernel takes
BIG_GUARD = 64 * 1024
FILL = 0x5A


@pytest.mark.parametrize("extra", [0, 1], ids=["max", "max_plus_1"])
@pytest.mark.parametrize("first", [2 ** 32 + 255, 2 ** 33], ids=["mod256_255", "mod256_0"])
def test_sum128_four_gib_edge(E, first, extra):
    """count = kSum128MaxCount runs prf_dmask_sum128_kernel with lane offsets up to 4 KiB below 2^32 bytes; one element more takes
    prf_chain_dmask_kernel.  About 30 GiB of HBM: plaintexts are filled with a byte pattern on the device, random values go only into
    the windows that are checked."""
    from flashe_amd._lib import FlasheError
    b, C, it, J = 128, 3, 17, 16
    count = SUM128_MAX + extra
    n = first + count + 1000
    idx = list(range(C))
    eng = E.Engine(KEY, b, device=0)
    bufs = []
    try:
        try:
            d_pts = [eng.alloc(8 * count) for _ in range(C)]
            bufs += d_pts
            cts = [Slab(eng, count, 16, guard=BIG_GUARD) for _ in range(C)]
            sm, out = Slab(eng, count, 16, guard=BIG_GUARD), Slab(eng, count, 16, guard=BIG_GUARD)
            bufs += [s.buf for s in cts + [sm, out]]
        except FlasheError as e:
            if e.code == -12:
                pytest.skip("needs about %.1f GiB of device memory (plaintexts, ciphertexts, sum, output and the chain's decrypt mask)"
                            % ((C * 8 + (C + 3) * 16) * count / 2 ** 30))
            raise
        rng = np.random.Generator(np.random.PCG64(first + extra))
        wins = [(0, 512), (2 ** 27 - 256, 512), (count - 512, 512), (count // 3 + 5, 256)]  # 16 * 2^27 = 2^31
        win_pts = {}
        for v in range(C):
            eng.memset_dev(d_pts[v], FILL, 8 * count)
            for k0, w in wins:
                vals = _rand_u64(rng, w)
                d_pts[v].upload_at(8 * k0, vals)
                win_pts[v, k0] = [int(x) for x in vals]
        eng.encrypt_batch_range_dev(it, idx, E.SCHEME_DOUBLE, n, J, first, count, d_pts, 1, [c.ptr() for c in cts], sm.ptr())
        eng.decrypt_range_dev(it, [idx[-1] + 1], [idx[0]], n, J, first, count, sm.ptr(), out.ptr())
        eng.sync()
        for s in cts + [sm, out]:
            s.check_guards()
        for k0, w in wins:
            js = range(first + k0, first + k0 + w)
            T = {i: [ref.term(KEY, it, i, n, J, b, j) for j in js] for i in range(C + 1)}
            want_ct = [[(win_pts[v, k0][k] + T[v][k] - T[v + 1][k]) % (1 << b) for k in range(w)] for v in range(C)]
            for v in range(C):
                assert cts[v].values(0, k0, k0 + w) == want_ct[v], (first, count, "ciphertext", v, k0)
            want_sum = _modsum(b, *want_ct)
            assert sm.values(0, k0, k0 + w) == want_sum, (first, count, "sum", k0)
            assert out.values(0, k0, k0 + w) == _modsum(b, *[win_pts[v, k0] for v in range(C)]), (first, count, "decrypt", k0)
        # between the windows every plaintext is the fill pattern: the decrypt there is 3 x the pattern (sampled)
        fill = int.from_bytes(bytes([FILL]) * 8, "little")
        for k in rng.integers(512, count - 512, 24):
            k = int(k)
            if any(k0 <= k < k0 + w for k0, w in wins):
                continue
            assert out.values(0, k, k + 1) == [3 * fill], (first, count, "decrypt of the fill", k)
    finally:
        for buf in bufs:
            buf.free()
        eng.close()


# ---------------------------------------------------------------------------------------------------------------- D. sparse near 2^32
@pytest.mark.parametrize("b", [20, 64, 128])
@pytest.mark.parametrize("J", [1, 16])
def test_sparse_positions_at_top_of_u32(E, b, J):
    eng = E.Engine(KEY, b, device=0)
    total, C, it = 2 ** 32 - 1, 3, 19
    span = eng.sparse_span()
    first = ((total - 1) // span - 1) * span           # the last two spans (the last one ends the vector)
    count = total - first
    rng = np.random.Generator(np.random.PCG64(b * 31 + J))
    locs = []
    for c in range(C):
        near0 = {c, 7 + c, 1000 + 3 * c}
        top = set(int(v) for v in rng.choice(count + 200, size=900 + 300 * c, replace=False) + (first - 200))
        top |= {total - 1, first} if c != 1 else {first - 1, first, first + 1}
        locs.append(np.array(sorted(p for p in near0 | top if p < total), dtype=np.uint32))
    assert max(int(l[-1]) for l in locs) == 2 ** 32 - 2
    ks = [len(l) for l in locs]
    idx = [5, 9, 2]
    zeros = [int(v) % (1 << b) for v in rng.integers(0, 2 ** 63, C)]
    pts = [_rand_u64(rng, k) for k in ks]
    dl = [eng.upload(l) for l in locs]
    dp = [eng.upload(p) for p in pts]
    bnd = eng.span_bounds(total, dl, ks)
    E8 = 8 * L(b)
    cts = [Slab(eng, k, E8) for k in ks]
    agg = Slab(eng, count, E8)
    eng.sparse_encrypt_aggregate_dev(it, idx, dl, ks, dp, 1, zeros, total, J, [c.ptr() for c in cts], agg.ptr(), bounds=bnd,
                                     position_range=(first, count))
    poison = int.from_bytes(bytes([POISON]) * E8, "little")
    held = [dict((int(p), q) for q, p in enumerate(l)) for l in locs]
    ct_want = []
    for c in range(C):
        got = cts[c].all_values()
        want = [(int(pts[c][q]) + ref.term(KEY, it, idx[c], ks[c], J, b, q)) % (1 << b) if int(locs[c][q]) >= first else poison
                for q in range(ks[c])]
        assert got == want, (b, J, "ciphertext", c)
        ct_want.append(want)
    want_agg = []
    for p in range(first, total):
        s = 0
        for c in range(C):
            q = held[c].get(p)
            s += zeros[c] if q is None else ct_want[c][q]
        want_agg.append(s % (1 << b))
    got_agg = agg.all_values()
    assert got_agg == want_agg, (b, J, "aggregate")

    out = Slab(eng, count, E8)
    eng.sparse_decrypt_dev(it, dl, ks, total, J, agg.ptr(), out.ptr(), bounds=bnd, position_range=(first, count))
    minus = ref.sparse_minus_mask(KEY, it, locs, J, b, range(first, total))
    assert out.all_values() == [(a - m) % (1 << b) for a, m in zip(got_agg, minus)], (b, J, "decrypt")
    del bnd
    eng.close()
