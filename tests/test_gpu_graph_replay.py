"""Graph replay with an iter shift (flashe_graph_launch_shifted) on every capturable PRF call.  Kernel arguments are frozen into a captured
graph; a replay is a NEW round only because every PRF kernel adds the device word te0[kIterShiftWord] to its frozen iter by hand
(device_common.h).  A kernel that forgets writes plausible ciphertexts under the previous round's mask streams, so every case here goes
through one helper (`replay`): run eagerly, poison, capture (nothing may run), then per shift r upload NEW inputs into the SAME buffers,
poison, replay and compare every output bit for bit with the CPU oracle called with iter + r; the same plaintext at r = 0 and r = 1 must
give different ciphertexts; an eager call afterwards runs at the plain iter again; after a key change the graph refuses to launch.

Single-stream captures on the table PRF only (no second stream, no bit-sliced or hybrid backend).  The host state that behaves
differently under a capture (span-bounds handles, prepared caches, scratch growth) and the synchronous calls that refuse one follow."""
import ctypes
import gc

import numpy as np
import pytest

import reduce_decrypt_ref as R

pytestmark = pytest.mark.gpu
KEY = bytes(range(32))
KEY2 = bytes(range(100, 132))
POISON = 0xA5
M32 = 0xFFFFFFFF
EINVAL = -22                                 # FLASHE_EINVAL (include/flashe.h)
SMALL, BIG = (0, 1, 5), (0, 3)             # shifts: small shapes, shapes above a million elements
SUMMED_MIN = 2_097_152                       # launch_prf_batch_sum: two 256-element tiles per wave of 256 CUs x 16 waves (test_gpu_index_limits.py)
MAX_IDX = 96                                 # kMaxIdx: prefixes per list and launch


@pytest.fixture(scope="module")
def E():
    from flashe_amd import engine
    return engine


def L(b):
    return 2 if b > 64 else 1


def bmask(b):
    return np.uint64((1 << min(b, 64)) - 1) if b < 64 else np.uint64(2 ** 64 - 1)


def rng_of(*seed):
    return np.random.Generator(np.random.PCG64([int(s) for s in seed]))


def rand_vec(rng, n, b):
    """[n, L] random elements below 2^b"""
    v = rng.integers(0, 2 ** 64, (n, L(b)), dtype=np.uint64)
    v[:, -1] &= np.uint64((1 << (b - 64 * (L(b) - 1))) - 1) if b % 64 else np.uint64(2 ** 64 - 1)
    return v


def raw(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _same(name, got, want, ctx):
    got, want = raw(got), raw(want)
    assert got.size == want.size, (name, ctx, got.size, want.size)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        pytest.fail("%s %r: %d of %d bytes differ, the first at byte %d" % (name, ctx, bad.size, got.size, bad[0]))


class Case:
    """The buffers of one captured sequence: ins / outs map a name to a device buffer; an output holds `nbytes` checked bytes."""

    def __init__(self, eng):
        self.eng, self.ins, self.outs = eng, {}, {}

    def inp(self, name, nbytes):
        self.ins[name] = self.eng.alloc(max(int(nbytes), 16))
        return self.ins[name]

    def out(self, name, nbytes):
        self.outs[name] = (self.eng.alloc(max(int(nbytes), 16)), int(nbytes))
        return self.outs[name][0]

    def upload(self, host):
        for name, arr in host.items():
            if raw(arr).size:
                self.ins[name].upload(raw(arr))

    def poison(self):
        for buf, nbytes in self.outs.values():
            self.eng.memset_dev(buf, POISON, max(nbytes, 16))

    def fetch(self):
        return {name: buf.download(np.uint8, nbytes) if nbytes else np.zeros(0, np.uint8) for name, (buf, nbytes) in self.outs.items()}

    def untouched(self):
        return all((got == POISON).all() for got in self.fetch().values())


def capture(eng, calls):
    gc.collect()        # (garbage of an earlier, failed test must not be freed during the capture: a hipFree on this thread would end it)
    eng.graph_begin()
    try:
        calls()
    except BaseException:
        try:
            eng.graph_end()
        except Exception:
            pass
        raise
    return eng.graph_end()


def refuses_after_a_key_change(E, eng, graphs):
    """Every graph carries the key schedule it was captured with: after set_key it refuses, and after the old key is set again it STILL
    refuses (the key epoch has moved on)."""
    for key in (KEY2, KEY):
        eng.set_key(key)
        for g in graphs:
            with pytest.raises(E.FlasheError):
                g.launch()
            with pytest.raises(E.FlasheError):
                g.launch(iter_shift=1)


def replay(E, case, it, calls, fill, want, shifts, ciphers, ctx, key_change=True):
    """calls(): the engine calls at iter `it`; fill(seed) -> {input name: array}; want(iter, host inputs) -> {output name: array};
    ciphers: the outputs that are ciphertexts of the inputs (the mask-reuse check)."""
    eng = case.eng
    host = fill(0)
    case.upload(host)
    calls()                                                       # 1. eagerly once: sizes the ctx scratch
    eng.sync()
    case.poison()                                                 # 2.
    g = capture(eng, calls)                                       # 3.
    eng.sync()
    assert case.untouched(), ("a capture records, it must not run anything", ctx)      # 4.
    for k, r in enumerate(shifts):                                # 5.
        host = fill(k + 1)
        case.upload(host)
        case.poison()
        g.launch(iter_shift=r)
        got, exp = case.fetch(), want((it + r) & M32, host)
        assert set(got) == set(exp), ctx
        for name in got:
            _same(name, got[name], exp[name], (ctx, "shift", r))
    # the same plaintext one round later: another mask stream, so another ciphertext
    case.poison()
    g.launch(iter_shift=0)
    ct0 = case.fetch()
    case.poison()
    g.launch(iter_shift=1)
    ct1 = case.fetch()
    for name in ciphers:
        assert not np.array_equal(ct0[name], ct1[name]), ("the replay at shift 1 reused the masks of shift 0", name, ctx)
    case.poison()                                                 # 6. the shift word is back at 0
    calls()
    got, exp = case.fetch(), want(it, host)
    for name in got:
        _same(name, got[name], exp[name], (ctx, "eager after the replays"))
    if key_change:
        refuses_after_a_key_change(E, eng, [g])
    return g


# ----------------------------------------------------------------------------------------------------------------------- 1. prefix lists
def _lists_case(E, oracle, b, n, J, it, shifts):
    """encrypt_dev (one add / one minus prefix: the job kernels) and decrypt_dev with 99 add and 97 minus prefixes: two launches of
    prf_wide_kernel (int_bits > 64) / prf_small_kernel (<= 64), the second one accumulating in place (prf_lists, abi.hip)."""
    eng = E.Engine(KEY, b, device=0)
    c = Case(eng)
    add, minus = list(range(200, 200 + MAX_IDX + 3)), list(range(5, 5 + MAX_IDX + 1))
    dpt, dagg = c.inp("pt", 8 * n), c.inp("agg", 8 * L(b) * n)
    dct, dout = c.out("ct", 8 * L(b) * n), c.out("dec", 8 * L(b) * n)

    def calls():
        eng.encrypt_dev(it, 3, E.SCHEME_DOUBLE, n, J, dpt, 1, dct)
        eng.decrypt_dev(it, add, minus, n, J, dagg, dout)

    def fill(seed):
        rng = rng_of(b, n, J, seed)
        return {"pt": rng.integers(0, 2 ** 64, n, dtype=np.uint64) & bmask(b), "agg": rand_vec(rng, n, b)}

    def want(i, h):
        return {"ct": oracle.encrypt(KEY, i, 3, "double", J, b, h["pt"]), "dec": oracle.decrypt(KEY, i, add, minus, J, b, h["agg"])}

    replay(E, c, it, calls, fill, want, shifts, ["ct", "dec"], (b, n, J, it))


@pytest.mark.parametrize("n,J", [(4_099, 16), (4_099, 1), (257, 16), (257, 1)])
@pytest.mark.parametrize("b", [128, 100, 64, 20])
def test_prefix_lists_longer_than_one_group(E, oracle, b, n, J):
    _lists_case(E, oracle, b, n, J, 7, SMALL)


@pytest.mark.parametrize("b", [128, 20])
def test_the_shifted_iter_wraps_like_the_kernels_uint32_add(E, oracle, b):
    """iter = 2^32 - 2 and a shift of 3: the round at (iter + 3) mod 2^32 = 1.  (The oracle takes any uint32 iter.)"""
    _lists_case(E, oracle, b, 257, 3, 2 ** 32 - 2, (3,))


# ----------------------------------------------------------------------------------------------------------------------- 2. - 4. the chains
@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("b", [128, 100])
def test_summed_chain(E, oracle, b, C):
    """encrypt_batch_sum_dev, double mask, one run of C clients on a vector that gives every wave two whole tiles (launch_prf_batch_sum)
    with a ragged last tile: the summed prf_chain_kernel (inside a capture the launch writes no decrypt mask, chain_dmask_begin)."""
    eng = E.Engine(KEY, b, device=0)
    n, J, it, idx = SUMMED_MIN + 2_851, 16, 7, list(range(2, 2 + C))
    assert (n + 255) // 256 >= 2 * eng.cu_count * 16, "the vector is too short for the summed launch on this device"
    c = Case(eng)
    dpt = [c.inp("pt%d" % v, 8 * n) for v in range(C)]
    dct = [c.out("ct%d" % v, 16 * n) for v in range(C)]
    dsum = c.out("sum", 16 * n)

    def calls():
        eng.encrypt_batch_sum_dev(it, idx, E.SCHEME_DOUBLE, n, J, dpt, 1, dct, dsum)

    def fill(seed):
        return {"pt%d" % v: rng_of(b, C, seed, v).integers(0, 2 ** 64, n, dtype=np.uint64) for v in range(C)}

    def want(i, h):
        cts = [oracle.encrypt(KEY, i, idx[v], "double", J, b, h["pt%d" % v]) for v in range(C)]
        out = {"ct%d" % v: cts[v] for v in range(C)}
        out["sum"] = oracle.aggregate_elem(cts, b)
        return out

    replay(E, c, it, calls, fill, want, BIG, ["ct%d" % v for v in range(C)] + ["sum"], (b, C, n))


def test_summed_chain_that_also_decrypts(E, oracle):
    """encrypt_batch_sum_decrypt_dev at int_bits 128 with one-limb plaintexts: prf_dec_sum128_kernel writes the ciphertexts, their sum and
    the decrypt of the sum with ([last + 1], [first])."""
    b, C = 128, 3
    eng = E.Engine(KEY, b, device=0)
    n, J, it, idx = SUMMED_MIN + 2_851, 16, 9, [4, 5, 6]
    assert (n + 255) // 256 >= 2 * eng.cu_count * 16
    c = Case(eng)
    dpt = [c.inp("pt%d" % v, 8 * n) for v in range(C)]
    dct = [c.out("ct%d" % v, 16 * n) for v in range(C)]
    dsum, ddec = c.out("sum", 16 * n), c.out("dec", 16 * n)

    def calls():
        eng.encrypt_batch_sum_decrypt_dev(it, idx, E.SCHEME_DOUBLE, n, J, dpt, 1, dct, dsum, ddec)

    def fill(seed):
        return {"pt%d" % v: rng_of(77, seed, v).integers(0, 2 ** 64, n, dtype=np.uint64) for v in range(C)}

    def want(i, h):
        cts = [oracle.encrypt(KEY, i, idx[v], "double", J, b, h["pt%d" % v]) for v in range(C)]
        out = {"ct%d" % v: cts[v] for v in range(C)}
        out["sum"] = oracle.aggregate_elem(cts, b)
        out["dec"] = oracle.decrypt(KEY, i, [idx[-1] + 1], [idx[0]], J, b, out["sum"])
        return out

    def want_checked(i, h):
        out = want(i, h)
        total = np.zeros(n, dtype=np.uint64)
        for v in range(C):
            total += h["pt%d" % v]
        assert np.array_equal(out["dec"][:, 0], total)            # (the reference round closes: the decrypt is the plaintext sum)
        return out

    replay(E, c, it, calls, fill, want_checked, BIG, ["ct0", "ct1", "ct2", "sum"], (b, C, n))


@pytest.mark.parametrize("b", [20, 32])
def test_compact_summed_chain(E, oracle, b):
    """encrypt_batch_sum_u32_dev: prf_small_chain_kernel with the sum in the compact layout.  n: the smallest vector small_cohort_admits /
    launch_small_chains take summed on this chip -- one chunk whose AES blocks (128 // b elements each) number 2 x 128 per wave of every
    workgroup, as the shapes of test_gpu_chain.py::test_compact_layout_at_compile_time_widths are derived -- and 7 more elements."""
    eng = E.Engine(KEY, b, device=0)
    assert eng.compact_supported()
    m, C, J, it, idx = 128 // b, 2, 1, 5, [3, 4]
    n = (2 * 128 * eng.cu_count * 16 - 1) * m + 1 + 7
    assert (n + m - 1) // m >= 2 * 128 * eng.cu_count * 16 and n < 2 ** 32
    c = Case(eng)
    dpt = [c.inp("pt%d" % v, 4 * n) for v in range(C)]
    dct = [c.out("ct%d" % v, 4 * n) for v in range(C)]
    dsum = c.out("sum", 4 * n)

    def calls():
        eng.encrypt_batch_sum_u32_dev(it, idx, E.SCHEME_DOUBLE, n, J, dpt, dct, dsum)

    def fill(seed):
        return {"pt%d" % v: rng_of(b, seed, v).integers(0, 2 ** b, n, dtype=np.uint64).astype(np.uint32) for v in range(C)}

    def want(i, h):
        cts = [oracle.encrypt(KEY, i, idx[v], "double", J, b, h["pt%d" % v].astype(np.uint64))[:, 0] for v in range(C)]
        out = {"ct%d" % v: cts[v].astype(np.uint32) for v in range(C)}
        out["sum"] = ((cts[0] + cts[1]) & bmask(b)).astype(np.uint32)
        return out

    replay(E, c, it, calls, fill, want, BIG, ["ct0", "ct1", "sum"], (b, n))


# ----------------------------------------------------------------------------------------------------------------------- 5. - 6. reduce + decrypt
@pytest.mark.parametrize("b,ie,oe", [(16, 4, 4), (16, 4, 8), (23, 4, 4), (23, 4, 8), (40, 8, 8)])
def test_small_reduce_decrypt(E, oracle, b, ie, oe):
    """The compact round: encrypt_batch_u32_dev, then aggregate_decrypt_u32_dev into uint32 or uint64 outputs -- int_bits <= 32 runs
    small_reduce_decrypt_split_kernel (launch_small_reduce_decrypt), and the one-limb layout at int_bits 40 small_reduce_decrypt_kernel.
    The shape of test_gpu_reduce_decrypt_edges.py's width group: chunk ends in mid tile, a partial last block, three tiles."""
    eng = E.Engine(KEY, b, device=0)
    (n, J), C, it, idx = R.width_shape(b), 3, 11, [2, 3, 4]
    c = Case(eng)
    dpt = [c.inp("pt%d" % v, ie * n) for v in range(C)]
    dct = [c.out("ct%d" % v, ie * n) for v in range(C)]
    dagg, dout = c.out("agg", oe * n), c.out("dec", oe * n)
    ity, oty = (np.uint32 if ie == 4 else np.uint64), (np.uint32 if oe == 4 else np.uint64)

    def calls():
        if ie == 4:
            eng.encrypt_batch_u32_dev(it, idx, E.SCHEME_DOUBLE, n, J, dpt, dct)
            eng.aggregate_decrypt_u32_dev(it, [5], [2], n, J, 0, n, dct, dagg, dout, out_elem_bytes=oe)
        else:
            eng.encrypt_batch_dev(it, idx, E.SCHEME_DOUBLE, n, J, dpt, 1, dct)
            eng.aggregate_decrypt_range_dev(it, [5], [2], n, J, 0, n, dct, dagg, dout)

    def fill(seed):
        return {"pt%d" % v: rng_of(b, ie, oe, seed, v).integers(0, 2 ** b, n, dtype=np.uint64).astype(ity) for v in range(C)}

    def want(i, h):
        cts = [oracle.encrypt(KEY, i, idx[v], "double", J, b, h["pt%d" % v].astype(np.uint64)) for v in range(C)]
        agg = oracle.aggregate_elem(cts, b)
        dec = oracle.decrypt(KEY, i, [5], [2], J, b, agg)
        total = sum(h["pt%d" % v].astype(np.uint64) for v in range(C)) & bmask(b)
        assert np.array_equal(dec[:, 0], total)
        out = {"ct%d" % v: cts[v][:, 0].astype(ity) for v in range(C)}
        out.update(agg=agg[:, 0].astype(oty), dec=dec[:, 0].astype(oty))
        return out

    replay(E, c, it, calls, fill, want, SMALL, ["ct0", "ct1", "ct2", "agg"], (b, ie, oe, n))


@pytest.mark.parametrize("C", [3, 64])
@pytest.mark.parametrize("b", [128, 65])
def test_wide_reduce_decrypt_over_a_pointer_table(E, oracle, b, C):
    """aggregate_decrypt_range_dev on a range with a non-zero `first`, C operands in allocations of their own: reduce_decrypt_ptrs_kernel
    (int_bits > 64, one add and one minus prefix, up to 64 operands anywhere in memory)."""
    eng = E.Engine(KEY, b, device=0)
    first, count, J, it = 1_237, 70_001, 5, 3
    n = first + count + 55
    c = Case(eng)
    dop = [c.inp("op%d" % v, 16 * count) for v in range(C)]
    dagg, dout = c.out("agg", 16 * count), c.out("dec", 16 * count)
    assert len({d.ptr for d in dop}) == C

    def calls():
        eng.aggregate_decrypt_range_dev(it, [C], [0], n, J, first, count, dop, dagg, dout)

    def fill(seed):
        return {"op%d" % v: rand_vec(rng_of(b, C, seed, v), count, b) for v in range(C)}

    masks = {}

    def want(i, h):
        if i not in masks:
            masks[i] = (np.ascontiguousarray(oracle.mask(KEY, i, C, n, J, b)[first:first + count]),
                        np.ascontiguousarray(oracle.mask(KEY, i, 0, n, J, b)[first:first + count]))
        agg = oracle.aggregate_elem([h["op%d" % v] for v in range(C)], b)
        return {"agg": agg, "dec": oracle.combine(b, agg, masks[i][0], masks[i][1])}

    replay(E, c, it, calls, fill, want, SMALL, ["dec"], (b, C, first, count))


# ----------------------------------------------------------------------------------------------------------------------- 7. job lists and ranges
@pytest.mark.parametrize("b", [128, 64, 20])
def test_job_lists_and_ranges(E, oracle, b):
    """prf_jobs_dev over ragged ranges (with and without an input, with and without a minus prefix), encrypt_batch_range_dev and
    mask_range_dev on a range that starts and ends inside a chunk: prf_wide_batch_kernel / the chained jobs at int_bits > 64,
    prf_small_jobs_kernel below."""
    eng = E.Engine(KEY, b, device=0)
    n, J, it, Lb = 9_999, 7, 21, L(b)
    jobs_spec = [(11, 12, 0, n, True), (13, None, 257, 4_001, False), (14, 15, 7_777, 2_222, True), (16, 17, 1_428, 1, True)]
    F, CNT, ridx = 1_301, 6_007, [4, 5, 9]
    c = Case(eng)
    jin = [c.inp("jin%d" % k, 8 * cnt) if has_in else None for k, (_, _, _, cnt, has_in) in enumerate(jobs_spec)]
    jout = [c.out("jout%d" % k, 8 * Lb * cnt) for k, (_, _, _, cnt, _) in enumerate(jobs_spec)]
    rpt = [c.inp("rpt%d" % v, 8 * CNT) for v in range(len(ridx))]
    rct = [c.out("rct%d" % v, 8 * Lb * CNT) for v in range(len(ridx))]
    rsum, rmask = c.out("rsum", 8 * Lb * CNT), c.out("rmask", 8 * Lb * CNT)
    jobs = [(a, m, f, cnt, jin[k], 1, jout[k]) for k, (a, m, f, cnt, _) in enumerate(jobs_spec)]

    def calls():
        eng.prf_jobs_dev(it, n, J, [j for j in jobs if j[1] is not None])        # (one call: jobs with a minus prefix, or without)
        eng.prf_jobs_dev(it, n, J, [j for j in jobs if j[1] is None])
        eng.encrypt_batch_range_dev(it, ridx, E.SCHEME_DOUBLE, n, J, F, CNT, rpt, 1, rct, rsum)
        eng.mask_range_dev(it, [7, 8], n, J, F, CNT, rmask)

    def fill(seed):
        rng = rng_of(b, seed)
        h = {"jin%d" % k: rng.integers(0, 2 ** 64, cnt, dtype=np.uint64) & bmask(b) for k, (_, _, _, cnt, has_in) in enumerate(jobs_spec) if has_in}
        h.update({"rpt%d" % v: rng.integers(0, 2 ** 64, CNT, dtype=np.uint64) & bmask(b) for v in range(len(ridx))})
        return h

    def want(i, h):
        mk = lambda idx, f, cnt: np.ascontiguousarray(oracle.mask(KEY, i, idx, n, J, b)[f:f + cnt])
        out = {}
        for k, (a, m, f, cnt, has_in) in enumerate(jobs_spec):
            src = h["jin%d" % k].reshape(cnt, 1) if has_in else np.zeros((cnt, 1), dtype=np.uint64)
            out["jout%d" % k] = oracle.combine(b, src, mk(a, f, cnt), mk(m, f, cnt) if m is not None else None)
        cts = []
        for v, idx in enumerate(ridx):
            full = np.zeros(n, dtype=np.uint64)
            full[F:F + CNT] = h["rpt%d" % v]
            cts.append(np.ascontiguousarray(oracle.encrypt(KEY, i, idx, "double", J, b, full)[F:F + CNT]))
            out["rct%d" % v] = cts[-1]
        out["rsum"] = oracle.aggregate_elem(cts, b)
        out["rmask"] = np.ascontiguousarray(oracle.mask_sum(KEY, i, [7, 8], n, J, b)[F:F + CNT])
        return out

    replay(E, c, it, calls, fill, want, SMALL, ["jout0", "jout1", "jout2", "jout3", "rct0", "rct1", "rct2", "rsum", "rmask"], (b, n))


# ----------------------------------------------------------------------------------------------------------------------- 8. the fused codec
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("b", [128, 20])
def test_fused_single_layer_codec(E, oracle, b, dtype):
    """quantize_encrypt_dev (the quantising front end of the PRF launch) and decrypt_unquantize_dev (its unquantising back end); the floats
    are compared as bytes with the oracle's decrypt + unquantize."""
    from flashe_amd.quantize import ACIQ
    eng = E.Engine(KEY, b, device=0)
    n, J, it, eb, C, Lb = 4_099, 7, 5, 16, 4, L(b)
    alpha = ACIQ(eb).get_alpha_gaus_direct(1.0)
    c = Case(eng)
    dx, du, dagg = c.inp("x", np.dtype(dtype).itemsize * n), c.inp("u", 8 * n), c.inp("agg", 8 * Lb * n)
    dct, dout = c.out("ct", 8 * Lb * n), c.out("floats", 8 * n)

    def calls():
        eng.quantize_encrypt_dev(it, 3, E.SCHEME_DOUBLE, n, J, dx, dtype == np.float64, alpha, eb, du, dct)
        eng.decrypt_unquantize_dev(it, [C], [0], n, J, dagg, alpha, eb, C, dout)

    def fill(seed):
        rs = np.random.RandomState(1000 * b + seed)
        x = (rs.standard_normal(n) * 1.3).astype(dtype)
        x[:3] = [0.0, 1e9, -1e9]
        agg = np.zeros((n, Lb), dtype=np.uint64)
        agg[:, 0] = (rs.randint(0, 2 ** 14, n).astype(np.uint64) * np.uint64(C)) & bmask(b)
        return {"x": x, "u": rs.random_sample(n), "agg": agg}

    def want(i, h):
        q = oracle.quantize(h["x"], alpha, eb, h["u"])
        dec = oracle.decrypt(KEY, i, [C], [0], J, b, h["agg"])
        return {"ct": oracle.encrypt(KEY, i, 3, "double", J, b, q), "floats": oracle.unquantize(dec, alpha, eb, C)}

    replay(E, c, it, calls, fill, want, SMALL, ["ct"], (b, dtype.__name__))


# ----------------------------------------------------------------------------------------------------------------------- 9. - 10. the sparse passes
def _sparse_lists(rng, total, ks):
    return [np.sort(rng.choice(total, k, replace=False)).astype(np.uint32) for k in ks]


def _sparse_want(oracle, i, b, idx, locs, pts, zeros, total, J, agg_in):
    """each client's compact ciphertext (single mask), the aggregate of the expanded uploads, and the decrypt of agg_in under the lists"""
    Lb = L(b)
    acc = np.zeros((total, Lb), dtype=np.uint64)
    cts = []
    for cidx, loc, pt, z in zip(idx, locs, pts, zeros):
        ct = oracle.encrypt(KEY, i, cidx, "single", J, b, pt) if len(pt) else np.zeros((0, Lb), dtype=np.uint64)
        cts.append(ct)
        zl = np.array([[z] + [0] * (Lb - 1)], dtype=np.uint64)
        acc = oracle.aggregate_elem([acc, oracle.expand_to_dense(total, loc, ct, zl, b)], b)
    dec = oracle.combine(b, agg_in, None, oracle.sparse_minus_mask(KEY, i, locs, total, J, b))
    return cts, acc, dec


@pytest.mark.parametrize("ranged", [False, True], ids=["whole", "position_range"])
@pytest.mark.parametrize("b", [128, 64, 20])
def test_sparse_round_with_a_bounds_handle(E, oracle, b, ranged):
    """sparse_encrypt_aggregate_dev + sparse_decrypt_dev with a span-bounds handle made BEFORE the capture (span_bounds_create is not
    capturable): span_prf_kernel at int_bits > 64, span_prf_small_kernel below; once more as one position range over the whole vector.
    The lists stay (the handle describes them); every replay gets new plaintexts and a new aggregate to decrypt."""
    eng = E.Engine(KEY, b, device=0)
    total, ks, J, it, Lb = 4 * eng.sparse_span() - 7, [500, 0, 500], 3, 6, L(b)
    idx, zeros = [7, 2, 11], [5, 6, 7]
    locs = _sparse_lists(rng_of(b, 1), total, ks)
    dl = [eng.upload(l) if l.size else eng.alloc(16) for l in locs]
    bnd = eng.span_bounds(total, dl, ks)
    c = Case(eng)
    dp = [c.inp("pt%d" % v, 8 * k) for v, k in enumerate(ks)]
    din = c.inp("agg_in", 8 * Lb * total)
    dct = [c.out("ct%d" % v, 8 * Lb * k) for v, k in enumerate(ks)]
    dagg, ddec = c.out("agg", 8 * Lb * total), c.out("dec", 8 * Lb * total)
    pr = (0, total) if ranged else None

    def calls():
        eng.sparse_encrypt_aggregate_dev(it, idx, dl, ks, dp, 1, zeros, total, J, dct, dagg, bounds=bnd, position_range=pr)
        eng.sparse_decrypt_dev(it, dl, ks, total, J, din, ddec, bounds=bnd, position_range=pr)

    def fill(seed):
        rng = rng_of(b, 2, seed)
        h = {"pt%d" % v: rng.integers(0, 2 ** 64, k, dtype=np.uint64) & bmask(b) for v, k in enumerate(ks)}
        h["agg_in"] = rand_vec(rng, total, b)
        return h

    def want(i, h):
        cts, agg, dec = _sparse_want(oracle, i, b, idx, locs, [h["pt%d" % v] for v in range(3)], zeros, total, J, h["agg_in"])
        out = {"ct%d" % v: cts[v] for v in range(3)}
        out.update(agg=agg, dec=dec)
        return out

    replay(E, c, it, calls, fill, want, SMALL, ["ct0", "ct2", "agg", "dec"], (b, total, ranged))
    eng.sync()


@pytest.mark.parametrize("b", [128, 20])
def test_sparse_masks(E, oracle, b):
    """sparse_double_masks_dev (sparse_edge_prf_kernel over the clients' run edges), sparse_dense_mask_dev from selectors and
    sparse_minus_mask_dev from sorted and from unsorted lists (the stream passes)."""
    eng = E.Engine(KEY, b, device=0)
    total, C, J, it, Lb = 20_011, 5, 3, 11, L(b)
    rng = rng_of(b, total)
    base = np.sort(rng.choice(total, total // 5, replace=False))
    locs = [np.unique(np.concatenate([base[rng.random(len(base)) < 0.7], rng.choice(total, len(base) // 10, replace=False)])).astype(np.uint32)
            for _ in range(C)]
    locs[2] = np.zeros(0, dtype=np.uint32)
    shuffled = [rng.permutation(l) for l in locs]
    ks = [len(l) for l in locs]
    ohs = []
    for l in locs:
        a = np.zeros(total, dtype=np.uint8)
        a[l] = 1
        ohs.append(a)
    minus = [ohs[v] & (1 - ohs[v - 1]) if v > 0 else ohs[v] for v in range(C)]
    add = [np.zeros(total, dtype=np.uint8)] + [ohs[v] & (1 - ohs[v + 1]) if v < C - 1 else ohs[v] for v in range(C)]
    dl = [eng.upload(l) if l.size else eng.alloc(16) for l in locs]
    du = [eng.upload(l) if l.size else eng.alloc(16) for l in shuffled]
    dsel = [eng.upload(s) for s in add]
    c = Case(eng)
    names = ["add", "minus", "dense", "mm_sorted", "mm_unsorted"]
    o = {name: c.out(name, 8 * Lb * total) for name in names}

    def calls():
        eng.sparse_double_masks_dev(it, dl, ks, total, o["add"], o["minus"])
        eng.sparse_dense_mask_dev(it, dsel, total, o["dense"])
        eng.sparse_minus_mask_dev(it, dl, ks, total, J, o["mm_sorted"], sorted_lists=True)
        eng.sparse_minus_mask_dev(it, du, ks, total, J, o["mm_unsorted"], sorted_lists=False)

    def want(i, h):
        wa = oracle.sparse_dense_mask(KEY, i, add, total, b)
        mm = oracle.sparse_minus_mask(KEY, i, locs, total, J, b)
        return {"add": wa, "minus": oracle.sparse_dense_mask(KEY, i, minus, total, b), "dense": wa, "mm_sorted": mm,
                "mm_unsorted": oracle.sparse_minus_mask(KEY, i, shuffled, total, J, b)}     # (entry q of a list takes term q of its stream)

    replay(E, c, it, calls, lambda seed: {}, want, SMALL, names, (b, total))
    eng.sync()


# ----------------------------------------------------------------------------------------------------------------------- 11. the precompute
@pytest.mark.parametrize("b", [128, 23])
def test_precompute_and_its_consumer_captured_together(E, oracle, b):
    """prepare_encrypt + encrypt_prepared_dev and prepare_decrypt + decrypt_prepared_dev in one capture: the mask jobs run at
    iter_next + r, the combines consume them, and both caches are spent after the capture as after the eager calls."""
    eng = E.Engine(KEY, b, device=0)
    n, J, it, C, Lb = 4_099, 5, 30, 6, L(b)
    c = Case(eng)
    dpt, dagg = c.inp("pt", 8 * n), c.inp("agg", 8 * Lb * n)
    dct, dout = c.out("ct", 8 * Lb * n), c.out("dec", 8 * Lb * n)

    def calls():
        eng.prepare_encrypt(it, 3, E.SCHEME_DOUBLE, n, J)
        eng.encrypt_prepared_dev(n, dpt, 1, dct)
        eng.prepare_decrypt(it, C, n, J)
        eng.decrypt_prepared_dev(it, [], [], n, J, dagg, dout)
        assert not eng.prepared_query(eng.PREPARED_ENCRYPT)[0] and not eng.prepared_query(eng.PREPARED_DECRYPT)[0]

    def fill(seed):
        rng = rng_of(b, 9, seed)
        return {"pt": rng.integers(0, 2 ** 64, n, dtype=np.uint64) & bmask(b), "agg": rand_vec(rng, n, b)}

    def want(i, h):
        return {"ct": oracle.encrypt(KEY, i, 3, "double", J, b, h["pt"]), "dec": oracle.decrypt(KEY, i, [C], [0], J, b, h["agg"])}

    replay(E, c, it, calls, fill, want, SMALL, ["ct", "dec"], (b, n))


# ======================================================================================================================= host state
@pytest.mark.parametrize("b", [128, 20])
def test_a_bounds_handles_lazy_reduce_table_inside_a_capture(E, oracle, b):
    """sparse_aggregate_dev(bounds=...) reads the plain-reduce table of the handle, which create / recompute leave to the first call that
    needs it (ensure_reduce_table, abi.hip).  Inside a capture that fill is only recorded: (1) without a replay an eager call must fill the
    table itself; (2) a replay fills and reduces; (3) after other lists of the same lengths went into the same buffers and
    bnd.recompute(), the replay reduces the new lists."""
    eng = E.Engine(KEY, b, device=0)
    total, ks, Lb = 4 * eng.sparse_span() - 7, [500, 0, 731], L(b)
    zeros = [3, 4, 5]

    def lists_and_values(seed):
        rng = rng_of(b, 40, seed)
        return _sparse_lists(rng, total, ks), [rand_vec(rng, k, b) for k in ks]

    def expected(locs, vals):
        acc = np.zeros((total, Lb), dtype=np.uint64)
        for loc, v, z in zip(locs, vals, zeros):
            acc = oracle.aggregate_elem([acc, oracle.expand_to_dense(total, loc, v, np.array([[z] + [0] * (Lb - 1)], dtype=np.uint64), b)], b)
        return acc

    locs, vals = lists_and_values(0)
    dl = [eng.alloc(4 * max(k, 4)) for k in ks]
    dv = [eng.alloc(8 * Lb * max(k, 2)) for k in ks]

    def upload(locs, vals):
        for d, a in list(zip(dl, locs)) + list(zip(dv, vals)):
            if a.size:
                d.upload(raw(a))

    upload(locs, vals)
    bnd = eng.span_bounds(total, dl, ks)
    out = eng.alloc(8 * Lb * total)

    def call():
        eng.sparse_aggregate_dev(total, dl, ks, dv, zeros, out, bounds=bnd)

    def result():
        return out.download(np.uint64, Lb * total).reshape(total, Lb)

    eng.memset_dev(out, POISON, out.nbytes)
    g = capture(eng, call)                                        # the FIRST use of the handle's reduce table is inside the capture
    eng.sync()
    assert (out.download(np.uint8, out.nbytes) == POISON).all()
    call()                                                        # (1) not replayed: the eager call fills the table itself
    _same("eager", result(), expected(locs, vals), (b, "the table a never-replayed graph never wrote"))
    eng.memset_dev(out, POISON, out.nbytes)
    g.launch()                                                    # (2)
    _same("replay", result(), expected(locs, vals), b)
    locs, vals = lists_and_values(1)                              # (3)
    upload(locs, vals)
    bnd.recompute(dl, ks)
    eng.memset_dev(out, POISON, out.nbytes)
    g.launch()
    _same("replay after recompute", result(), expected(locs, vals), b)
    eng.memset_dev(out, POISON, out.nbytes)
    call()
    _same("eager after recompute", result(), expected(locs, vals), b)
    refuses_after_a_key_change(E, eng, [g])


def _growth_refused(E, oracle, eng, b, grow, out, warm, n_small):
    """Inside a capture next to an encrypt: `grow` needs more ctx scratch than `warm` gave it -- refused, nothing written, the capture
    ends, and the graph of the other call replays correctly."""
    J, it = 3, 8
    pt = rng_of(b, n_small).integers(0, 2 ** 64, n_small, dtype=np.uint64) & bmask(b)
    dpt, dct = eng.upload(pt), eng.alloc(8 * L(b) * n_small)
    warm()
    eng.sync()
    eng.memset_dev(out, POISON, out.nbytes)
    eng.memset_dev(dct, POISON, dct.nbytes)
    gc.collect()
    eng.graph_begin()
    try:
        eng.encrypt_dev(it, 2, E.SCHEME_DOUBLE, n_small, J, dpt, 1, dct)
        with pytest.raises(E.FlasheError, match="scratch memory cannot grow"):
            grow()
    finally:
        g = eng.graph_end()                                       # the capture is still able to end
    g.launch(iter_shift=2)
    eng.sync()
    assert (out.download(np.uint8, out.nbytes) == POISON).all(), "the refused call wrote (or recorded a write)"
    _same("ct", dct.download(np.uint64, L(b) * n_small), oracle.encrypt(KEY, it + 2, 2, "double", J, b, pt), (b, "the rest of the graph"))
    grow()                                                        # fine outside a capture
    eng.sync()
    assert not (out.download(np.uint8, out.nbytes) == POISON).all()


def test_scratch_growth_is_refused_in_every_family(E, oracle):
    """One call of the dense PRF, the sparse and the codec family each; all three stage through the ctx's stream scratch."""
    small, big = 300, 5_000
    # dense PRF: a reduce + decrypt with two add prefixes at int_bits 64 keeps its aggregate in ctx scratch when agg_out is left out
    eng = E.Engine(KEY, 64, device=0)
    ops = [eng.upload(rng_of(v).integers(0, 2 ** 64, big, dtype=np.uint64)) for v in range(3)]
    out = eng.alloc(8 * big)
    _growth_refused(E, oracle, eng, 64, lambda: eng.aggregate_decrypt_range_dev(4, [3, 7], [0], big, 3, 0, big, ops, None, out), out,
                    lambda: eng.aggregate_decrypt_range_dev(4, [3, 7], [0], small, 3, 0, small, ops, None, out), small)
    # sparse: the dense mask from selectors stages each stream in ctx scratch
    eng = E.Engine(KEY, 128, device=0)
    sel = [eng.upload((rng_of(9, v).random(big) < 0.3).astype(np.uint8)) for v in range(2)]
    out = eng.alloc(16 * big)
    _growth_refused(E, oracle, eng, 128, lambda: eng.sparse_dense_mask_dev(4, sel, big, out), out,
                    lambda: eng.sparse_dense_mask_dev(4, sel, small, out), small)
    # codec: the fused decrypt + unquantise accumulates all but the last group of a long prefix list in ctx scratch
    eng = E.Engine(KEY, 128, device=0)
    agg, out = eng.upload(rand_vec(rng_of(5), big, 128)), eng.alloc(8 * big)
    add = list(range(100, 100 + MAX_IDX + 1))
    _growth_refused(E, oracle, eng, 128, lambda: eng.decrypt_unquantize_dev(4, add, [0], big, 3, agg, 3.5, 16, 4, out), out,
                    lambda: eng.decrypt_unquantize_dev(4, add, [0], small, 3, agg, 3.5, 16, 4, out), small)


# ======================================================================================================================= clean refusals
def test_synchronous_calls_are_refused_in_a_capture(E, oracle):
    """Every exported call that waits for the ctx stream or copies to or from host memory on it, between graph_begin and graph_end on an
    engine of its own: FLASHE_EINVAL with a message before the stream is touched, nothing written, the capture ends, and the graph of the
    remaining calls replays.  flashe_prepared_discard keeps its documented behaviour: it marks the cache invalid and frees nothing."""
    b, n, J, it = 128, 1_000, 3, 4
    eng = E.Engine(KEY, b, device=0)
    lib, h = eng._lib, eng._h
    pt = rng_of(1).integers(0, 2 ** 64, n, dtype=np.uint64)
    dpt, dct = eng.upload(pt), eng.alloc(16 * n)
    x = eng.upload(np.arange(n, dtype=np.float64))
    dst = eng.alloc(16 * n)
    host_in, host_out = np.full(2 * n, 7, dtype=np.uint64), np.full(2 * n, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    mean, std = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
    eng.prepare_decrypt(it, 3, n, J)
    idx1 = (ctypes.c_uint32 * 1)(5)
    eng.memset_dev(dst, POISON, dst.nbytes)
    eng.memset_dev(dct, POISON, dct.nbytes)
    eng.sync()
    refusals = {
        "flashe_mean_std_dev": lambda: lib.flashe_mean_std_dev(h, n, x.ptr, 1, ctypes.byref(mean), ctypes.byref(std)),
        "flashe_sync": lambda: lib.flashe_sync(h),
        "flashe_memcpy_h2d": lambda: lib.flashe_memcpy_h2d(h, dst.ptr, host_in.ctypes.data, host_in.nbytes),
        "flashe_memcpy_d2h": lambda: lib.flashe_memcpy_d2h(h, host_out.ctypes.data, dpt.ptr, 8 * n),
        "flashe_selftest": lambda: lib.flashe_selftest(h),
        "flashe_ctx_set_key": lambda: lib.flashe_ctx_set_key(h, (ctypes.c_uint8 * 32)(*KEY2)),
        "flashe_mask (host-pointer twin)": lambda: lib.flashe_mask(h, it, idx1, 1, n, J, host_out.ctypes.data),
        "flashe_encrypt (host-pointer twin)": lambda: lib.flashe_encrypt(h, it, 5, E.SCHEME_DOUBLE, n, J, host_in.ctypes.data, 1, host_out.ctypes.data),
    }
    gc.collect()
    eng.graph_begin()
    try:
        eng.encrypt_dev(it, 2, E.SCHEME_DOUBLE, n, J, dpt, 1, dct)
        rcs = {}
        for name, call in refusals.items():
            rcs[name] = (call(), lib.flashe_last_error(h))
        with pytest.raises(E.FlasheError):
            eng.sync()                                            # (the Python layer raises it)
        with pytest.raises(E.FlasheError):
            dct.download(np.uint64, 2)
        eng.prepared_discard(eng.PREPARED_DECRYPT)                # marks invalid, frees nothing, touches no stream
        assert not eng.prepared_query(eng.PREPARED_DECRYPT)[0]
    finally:
        g = eng.graph_end()                                       # every refusal left the capture able to end
    for name, (rc, msg) in rcs.items():
        assert rc == EINVAL, (name, rc)
        assert b"not capturable" in msg, (name, msg)
    assert mean.value == -1.0 and std.value == -1.0
    assert (host_out == np.uint64(0x5A5A5A5A5A5A5A5A)).all()
    eng.sync()                                                    # works again after the capture
    assert (dst.download(np.uint8, dst.nbytes) == POISON).all() and (dct.download(np.uint8, dct.nbytes) == POISON).all()
    g.launch(iter_shift=1)                                        # the graph of the remaining call, under the key the capture began with
    _same("ct", dct.download(np.uint64, 2 * n), oracle.encrypt(KEY, it + 1, 2, "double", J, b, pt), "after the refusals")
    eng.selftest()
    m, s = eng.mean_std_dev(n, x, True)
    assert m == pytest.approx((n - 1) / 2)
    refuses_after_a_key_change(E, eng, [g])
