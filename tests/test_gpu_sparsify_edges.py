"""The top-k sparsifier's kernels (flashe_amd/csrc/sparsify.hip) against the NumPy reference of tests/sparsify_ref.py, byte for byte -- no
tolerance anywhere -- through its four entry points: flashe_sparsify, flashe_sparsify_batch[_dev], flashe_sparsify_tensors_dev and
flashe_sparsify_cohort_tensors_dev.  The inputs are that module's builders (edge bit patterns, concentrated digits, ties, +-0,
subnormals, inf) at sizes around the lane / wave / block / trip boundaries, a sweep of the tie quota over every position of a block, a
layer whose block scan needs its carry, the packed locations at every width, and the k == 0 rule.  tests/test_sparsify_ref_host.py
holds the reference itself to the C oracle and to the reference project's golden rounds, without a GPU."""
import functools

import numpy as np
import pytest

import sparsify_ref as sr

pytestmark = pytest.mark.gpu

KEY = bytes(range(32))
SENT = 0xA5                                    # what every output buffer holds before a call: bytes no call may touch keep it
TIE_N = 9221                                   # 9 blocks + 5 elements, three trips of four blocks
TIE_SKIPS = list(range(0, 1031)) + list(range(4093, 4100)) + list(range(8189, 8196)) + [TIE_N - 1, TIE_N]
TIE_SUBSET = [0, 1, 2, 3, 4, 5, 255, 256, 257, 258, 259, 260, 261, 511, 512, 513, 767, 768, 1019, 1020, 1021, 1022, 1023, 1024, 1025, 1026,
              1027, 1028, 1029, 1030, 4093, 4095, 4096, 4097, 4099, 8189, 8191, 8192, 8193, 8195, TIE_N - 1, TIE_N]


@pytest.fixture(scope="module")
def E():
    from flashe_amd import engine
    return engine


@pytest.fixture(scope="module")
def eng(E):
    return E.Engine(KEY, 128, device=0)


def _codes():
    from flashe_amd import _lib
    return {"f32": _lib.TENSOR_F32, "f64": _lib.TENSOR_F64, "f16": _lib.TENSOR_F16, "bf16": _lib.TENSOR_BF16}


def _cls(kind):
    return "f64" if kind == "f64" else "f32"


# ---------------------------------------------------------------------------------------------------------------- cases and expectations
@functools.lru_cache(maxsize=2)
def _builder_cases(kinds):
    """Every builder at every size with every k it names, the kind cycling over `kinds`: [(storage layer, residual, k)], and the reference
    results of round 1 (from the builder's residual) and round 2 (the same layers on the residuals round 1 left)."""
    cases, i = [], 0
    for bi, build in enumerate(sr.BUILDERS):
        for n in sr.GPU_SIZES:
            kind = kinds[i % len(kinds)]
            i += 1
            layer, res, ks = build(kind, n, 1000 * bi + n)
            cases += [(layer, res, k) for k in ks]
    want1 = [sr.topk_ref(l, k, r) for l, r, k in cases]
    want2 = [sr.topk_ref(l, k, w[2]) for (l, _r, k), w in zip(cases, want1)]
    for c in cases:
        c[0].setflags(write=False)
        c[1].setflags(write=False)
    return cases, (want1, want2)


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        for name, a, b in zip(("loc", "vals", "residual"), g, w):
            if a is None and name == "residual":
                continue
            a = np.asarray(a)
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, "case", i, name, "n", w[2].size, "k", len(w[0]),
                                                                                               "first difference at", _first_diff(a, b))


def _first_diff(a, b):
    if a.shape != b.shape:
        return "shapes", a.shape, b.shape
    ua, ub = a.view(np.uint8).reshape(a.size, -1), b.view(np.uint8).reshape(b.size, -1)
    bad = np.flatnonzero((ua != ub).any(axis=1))
    return (int(bad[0]), a[bad[0]], b[bad[0]], "of", bad.size) if bad.size else None


# ---------------------------------------------------------------------------------------------------------------- the entry points
def _run_single(eng, cases, residuals):
    return [eng.sparsify(l, k, r) for (l, _r, k), r in zip(cases, residuals)]


def _run_batch(eng, cases, residuals):
    return eng.sparsify_batch([c[0] for c in cases], [c[2] for c in cases], residuals)


def _run_batch_dev(eng, cases, residuals):
    """flashe_sparsify_batch_dev on raw bytes: layers back to back (odd sizes put the next layer off 16-byte alignment)."""
    dt = cases[0][0].dtype
    ns, ks = [c[0].size for c in cases], [c[2] for c in cases]
    K = sum(ks)
    dx = eng.upload(np.concatenate([c[0] for c in cases]))
    dr = None if residuals is None else eng.upload(np.concatenate(residuals))
    dl, dv = eng.upload(np.full(4 * K + 64, SENT, np.uint8)), eng.upload(np.full(dt.itemsize * K + 64, SENT, np.uint8))
    eng.sparsify_batch_dev(ns, ks, dx, dt == np.float64, dr, dl, dv)
    loc, vals = dl.download(np.uint8), dv.download(np.uint8)
    assert (loc[4 * K:] == SENT).all() and (vals[dt.itemsize * K:] == SENT).all()
    loc, vals = loc[:4 * K].view(np.uint32), vals[:dt.itemsize * K].view(dt)
    res = None if dr is None else dr.download(dt, sum(ns))
    out, o, q = [], 0, 0
    for n, k in zip(ns, ks):
        out.append((loc[q:q + k], vals[q:q + k], None if res is None else res[o:o + n]))
        o, q = o + n, q + k
    return out


def _layout(ns, ks, classes):
    """Byte offsets of the layers' residuals and kept values in a client's block (include/flashe.h): each aligned to its compute size."""
    roff, voff, r, v = [], [], 0, 0
    for n, k, c in zip(ns, ks, classes):
        cs = 8 if c == "f64" else 4
        r, v = (r + cs - 1) // cs * cs, (v + cs - 1) // cs * cs
        roff.append(r)
        voff.append(v)
        r, v = r + n * cs, v + k * cs
    return roff, voff, r, v


def _run_tensors(eng, clients, ks, residuals, bits=0, cohort=False):
    """flashe_sparsify_tensors_dev (one client) or flashe_sparsify_cohort_tensors_dev: clients[c][l] = client c's storage layer l,
    residuals[c][l] its compute-type residual (residuals None = NULL).  Every layer lies one element past a 16-byte boundary; the
    clients' blocks are strided wider than they need; every byte that no output covers must come back untouched.
    -> per client ([(model-wide loc, vals, new residual or None) per layer], packed limbs or None)."""
    codes = _codes()
    C, L = len(clients), len(ks)
    ns = [l.size for l in clients[0]]
    classes = [_cls(sr.kind_of(l)) for l in clients[0]]
    assert all([l.size for l in cl] == ns and [_cls(sr.kind_of(l)) for l in cl] == classes for cl in clients)
    starts = [int(v) for v in np.concatenate([[0], np.cumsum(ns)[:-1]])]
    total, K = sum(ns), sum(ks)
    roff, voff, rbytes, vbytes = _layout(ns, ks, classes)
    # the sources: one upload, every layer at 16 a + its element size
    offs, at = [], 0
    for cl in clients:
        row = []
        for l in cl:
            at = (at + 15) // 16 * 16 + l.itemsize
            row.append(at)
            at += l.nbytes
        offs.append(row)
    src = np.zeros(at + 64, np.uint8)
    for cl, row in zip(clients, offs):
        for l, o in zip(cl, row):
            src[o:o + l.nbytes] = l.view(np.uint8)
    dsrc = eng.upload(src)
    if cohort:
        rstride, vstride, lstride = (rbytes + 7) // 8 * 8 + 64, (vbytes + 7) // 8 * 8 + 40, K + 7
    else:
        assert C == 1
        rstride, vstride, lstride = rbytes, vbytes, K
    n_limbs = (K * bits + 63) // 64 if bits else 0
    pstride = n_limbs + 3 if cohort else n_limbs
    dres = None
    if residuals is not None:
        rb = np.full(C * rstride + 64, SENT, np.uint8)
        for c in range(C):
            for l in range(L):
                r = residuals[c][l]
                assert r.dtype == sr.compute_dtype(classes[l]) and r.size == ns[l]
                rb[c * rstride + roff[l]:c * rstride + roff[l] + r.nbytes] = r.view(np.uint8)
        dres = eng.upload(rb)
    dloc = eng.upload(np.full(4 * C * lstride + 64, SENT, np.uint8))
    dval = eng.upload(np.full(C * vstride + 64, SENT, np.uint8))
    dpk = eng.upload(np.full(8 * C * pstride + 64, SENT, np.uint8)) if bits else None
    if cohort:
        table = [(s, codes[c]) for s, c in zip(starts, classes)]
        srcs = [[dsrc.ptr + o for o in row] for row in offs]
        dts = [[codes[sr.kind_of(l)] for l in cl] for cl in clients]
        eng.sparsify_cohort_tensors_dev(total, table, ks, srcs, dts, dres, rstride, dloc, lstride, dval, vstride, dpk, pstride, bits)
    else:
        eng.sparsify_tensors_dev(total, [(s, dsrc.ptr + o, codes[sr.kind_of(l)]) for s, o, l in zip(starts, offs[0], clients[0])], ks, dres, dloc,
                                 dval, dpk, bits)
    loc, val = dloc.download(np.uint8), dval.download(np.uint8)
    res = None if dres is None else dres.download(np.uint8)
    pk = None if dpk is None else dpk.download(np.uint8)
    assert dsrc.download(np.uint8).tobytes() == src.tobytes(), "a source was written"
    seen_l, seen_v = np.zeros(loc.size, bool), np.zeros(val.size, bool)
    seen_r = None if res is None else np.zeros(res.size, bool)
    seen_p = None if pk is None else np.zeros(pk.size, bool)
    out = []
    for c in range(C):
        rows, q = [], 0
        for l in range(L):
            ct = sr.compute_dtype(classes[l])
            a = 4 * (c * lstride + q)
            b = c * vstride + voff[l]
            got_l, got_v = loc[a:a + 4 * ks[l]].view(np.uint32), val[b:b + ct.itemsize * ks[l]].view(ct)
            seen_l[a:a + 4 * ks[l]] = True
            seen_v[b:b + ct.itemsize * ks[l]] = True
            got_r = None
            if res is not None:
                d = c * rstride + roff[l]
                got_r = res[d:d + ct.itemsize * ns[l]].view(ct)
                seen_r[d:d + ct.itemsize * ns[l]] = True
            rows.append((got_l, got_v, got_r))
            q += ks[l]
        limbs = None
        if pk is not None:
            limbs = pk[8 * c * pstride:8 * (c * pstride + n_limbs)].view(np.uint64)
            seen_p[8 * c * pstride:8 * (c * pstride + n_limbs)] = True
        out.append((rows, limbs))
    for name, buf, seen in (("loc", loc, seen_l), ("vals", val, seen_v), ("residual", res, seen_r), ("packed", pk, seen_p)):
        if buf is not None:
            assert (buf[~seen] == SENT).all(), (name, "bytes outside every output were written", np.flatnonzero(buf[~seen] != SENT)[:8])
    return out


def _model_wide(want, ns):
    """The reference results with the layers' dense starts added to the locations."""
    starts = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.uint32)
    return [(w[0] + s, w[1], w[2]) for w, s in zip(want, starts)]


# ---------------------------------------------------------------------------------------------------------------- a. the builders
@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_builders_one_layer_at_a_time(eng, kind):
    """flashe_sparsify on every builder, size and k; two rounds, the second on the residuals the first left; then with no residual."""
    cases, wants = _builder_cases((kind,))
    res = [c[1] for c in cases]
    for rnd in range(2):
        got = _run_single(eng, cases, res)
        _assert_same(got, wants[rnd], ("sparsify", kind, "round", rnd))
        res = [g[2] for g in got]
    got = _run_single(eng, cases[::7], [None] * len(cases[::7]))
    assert all(g[2] is None for g in got)
    _assert_same(got, [sr.topk_ref(l, k, None) for l, _r, k in cases[::7]], ("sparsify, no residual", kind))


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_builders_back_to_back_in_one_batch(eng, kind, form):
    """flashe_sparsify_batch / _dev: all of them as the layers of ONE call -- layer starts off 16-byte alignment, layer changes inside a trip."""
    cases, wants = _builder_cases((kind,))
    run = _run_batch if form == "host" else _run_batch_dev
    res = [c[1] for c in cases]
    for rnd in range(2):
        got = run(eng, cases, res)
        _assert_same(got, wants[rnd], ("sparsify_batch", form, kind, "round", rnd))
        res = [g[2] for g in got]
    got = run(eng, cases, None)
    assert all(g[2] is None for g in got)
    _assert_same(got, [sr.topk_ref(l, k, None) for l, _r, k in cases], ("sparsify_batch, no residual", form, kind))


@pytest.mark.parametrize("kinds", [("f32",), ("f64",), ("f16",), ("bf16",), ("f32", "f64", "f16", "bf16", "f64")], ids=lambda k: "+".join(k))
def test_builders_as_caller_owned_tensors(eng, kinds):
    """flashe_sparsify_tensors_dev: every storage dtype and a model that mixes them (the float64 layers sorted behind the others inside),
    the layers one element past an aligned address."""
    cases, wants = _builder_cases(kinds)
    layers, ks = [c[0] for c in cases], [c[2] for c in cases]
    ns = [l.size for l in layers]
    res = [c[1] for c in cases]
    for rnd in range(2):
        (got, _pk), = _run_tensors(eng, [layers], ks, [res])
        _assert_same(got, _model_wide(wants[rnd], ns), ("sparsify_tensors", kinds, "round", rnd))
        res = [g[2] for g in got]
    (got, _pk), = _run_tensors(eng, [layers], ks, None)
    _assert_same(got, _model_wide([sr.topk_ref(l, k, None) for l, _r, k in cases], ns), ("sparsify_tensors, no residual", kinds))


@functools.lru_cache(maxsize=None)
def _cohort_cases(mixed):
    """Three clients of one shape: row (builder b, size) keeps k = the row's turn of {0, 1, n // 2, n - 1, n}; client c's data come from
    builder b + c.  Client 0 stores float32, client 1 bfloat16 under every other float32 row, client 2 float16 under all of them; in the
    mixed shape every fourth row is float64 for everybody."""
    B = len(sr.BUILDERS)
    ks, clients, residuals = [], [[], [], []], [[], [], []]
    row = 0
    for b in range(B):
        for n in sr.GPU_SIZES:
            f64 = mixed and row % 4 == 3
            ks.append([0, 1, n // 2, n - 1, n][row % 5])
            for c, kind in enumerate(("f32", "bf16" if row % 2 else "f32", "f16")):
                layer, res, _ks = sr.BUILDERS[(b + c) % B]("f64" if f64 else kind, n, 7000 * c + 1000 * b + n)
                clients[c].append(layer)
                residuals[c].append(res)
            row += 1
    want1 = [[sr.topk_ref(l, k, r) for l, k, r in zip(cl, ks, rs)] for cl, rs in zip(clients, residuals)]
    want2 = [[sr.topk_ref(l, k, w[2]) for l, k, w in zip(cl, ks, ws)] for cl, ws in zip(clients, want1)]
    return ks, clients, residuals, (want1, want2)


@pytest.mark.parametrize("mixed", [False, True], ids=["f32_class", "mixed"])
def test_builders_through_a_cohort(eng, mixed):
    """flashe_sparsify_cohort_tensors_dev: C = 3, strides wider than a block, 16-bit storage under float32 rows, the padding untouched."""
    ks, clients, residuals, wants = _cohort_cases(mixed)
    ns = [l.size for l in clients[0]]
    res = residuals
    for rnd in range(2):
        got = _run_tensors(eng, clients, ks, res, cohort=True)
        for c in range(3):
            _assert_same(got[c][0], _model_wide(wants[rnd][c], ns), ("sparsify_cohort", mixed, "client", c, "round", rnd))
        res = [[g[2] for g in rows] for rows, _pk in got]
    got = _run_tensors(eng, clients, ks, None, cohort=True)
    for c in range(3):
        _assert_same(got[c][0], _model_wide([sr.topk_ref(l, k, None) for l, k in zip(clients[c], ks)], ns), ("sparsify_cohort, no residual", mixed, c))


# ---------------------------------------------------------------------------------------------------------------- b. the tie quota
@functools.lru_cache(maxsize=None)
def _tie_sweep():
    layer, res = sr.all_tied(TIE_N)
    return layer, res, {s: sr.topk_ref(layer, TIE_N - s, res) for s in TIE_SKIPS}


def test_tie_quota_ends_at_every_position_of_a_block():
    """(the reference side of the sweep: with every element tied, exactly the `skip` lowest indices stay out)"""
    _layer, _res, want = _tie_sweep()
    for s in TIE_SKIPS:
        assert np.array_equal(want[s][0], np.arange(s, TIE_N, dtype=np.uint32))


def test_tie_quota_sweep_in_one_batch(eng):
    """An all-tied layer of 9 blocks + 5 elements, one layer per k of ONE flashe_sparsify_batch call: skip = n - k ends inside a lane's
    four elements, at every wave, block and trip boundary."""
    layer, res, want = _tie_sweep()
    cases = [(layer, res, TIE_N - s) for s in TIE_SKIPS]
    _assert_same(_run_batch(eng, cases, [res] * len(cases)), [want[s] for s in TIE_SKIPS], "tie sweep, batch")


def test_tie_quota_subset_one_layer_and_tensors(eng):
    layer, res, want = _tie_sweep()
    assert set(TIE_SUBSET) <= set(TIE_SKIPS) and 38 <= len(TIE_SUBSET) <= 44
    cases = [(layer, res, TIE_N - s) for s in TIE_SUBSET]
    w = [want[s] for s in TIE_SUBSET]
    _assert_same(_run_single(eng, cases, [res] * len(cases)), w, "tie sweep, one layer")
    (got, _pk), = _run_tensors(eng, [[layer] * len(cases)], [c[2] for c in cases], [[res] * len(cases)])
    _assert_same(got, _model_wide(w, [TIE_N] * len(cases)), "tie sweep, tensors")


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_ties_with_riders(eng, kind):
    """0.5 everywhere, 3.0 at every 37th index: the riders are all above the threshold, t = 0 .. 260 ties join them."""
    ts = list(range(261))
    layer, res, _ks = sr.build_riders(kind, TIE_N, 77, ts=ts)
    cnt = sr.riders_count(TIE_N)
    cases = [(layer, res, cnt + t) for t in ts]
    want = [sr.topk_ref(layer, k, res) for _l, _r, k in cases]
    _assert_same(_run_batch(eng, cases, [res] * len(cases)), want, ("riders, batch", kind))
    (got, _pk), = _run_tensors(eng, [[layer] * len(cases)], [c[2] for c in cases], [[res] * len(cases)])
    _assert_same(got, _model_wide(want, [TIE_N] * len(cases)), ("riders, tensors", kind))


# ---------------------------------------------------------------------------------------------------------------- c. the scan's carry
def test_quota_ends_beyond_the_scan_chunk(eng):
    """A float32 layer of 1024 * 1024 + 3 * 1024 + 5 elements (1,028 blocks: the per-layer scan needs a second chunk and its carry), more than
    half of them tied at the threshold; the quota ends in block 1,025 and, for comparison, in block 3."""
    n = 1024 * 1024 + 3 * 1024 + 5
    rng = np.random.Generator(np.random.PCG64(31))
    mag = np.where(np.arange(n) % 3 != 0, 1.0, np.where(np.arange(n) % 15 == 0, 2.0, 0.25))
    layer = (mag * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    res = (np.arange(n) % 4093).astype(np.float32) * np.float32(0.5)
    tied = np.flatnonzero(mag == 1.0)
    n_gt = int((mag == 2.0).sum())
    assert 2 * tied.size > n
    for edge in (1025 * 1024 + 301, 3 * 1024 + 2):
        skip = int(np.searchsorted(tied, edge))                                 # the ties below `edge` stay out
        k = n_gt + tied.size - skip
        want = sr.topk_ref(layer, k, res)
        assert want[0][want[0] >= edge].size == k - int((mag[:edge] == 2.0).sum())
        _assert_same(_run_single(eng, [(layer, res, k)], [res]), [want], ("carry, one layer", edge))
        (got, _pk), = _run_tensors(eng, [[layer]], [k], [[res]])
        _assert_same(got, [want], ("carry, tensors", edge))


# ---------------------------------------------------------------------------------------------------------------- d. packed locations
def _pack_model(seed):
    sizes = (1000, 7, 1024, 969)
    layers, res = [], []
    for i, n in enumerate(sizes):
        l, r, _ks = sr.build_pool("f32", n, seed + i)
        layers.append(l)
        res.append(r)
    return sizes, layers, res


@pytest.mark.parametrize("ks", [(0, 1, 0, 0), (20, 3, 40, 1), (10, 7, 19, 1), (1000, 7, 1024, 969)], ids=["K1", "K64", "K37", "Kn"])
def test_packed_locations_at_every_width(eng, ks):
    """`_to_bytes(loc, bits)` for bits from n.bit_length() to 32, one model and a cohort of two: K bits a multiple of 64 (K = 64) and not,
    K = 1, K = n; the limbs behind the last one untouched."""
    sizes, layers, res = _pack_model(40)
    _s, layers2, res2 = _pack_model(50)
    n = sum(sizes)
    want = [_model_wide([sr.topk_ref(l, k, r) for l, k, r in zip(ls, ks, rs)], sizes) for ls, rs in ((layers, res), (layers2, res2))]
    locs = [np.concatenate([w[0] for w in ws]) for ws in want]
    assert n.bit_length() == 12 and len(locs[0]) == sum(ks)
    for bits in range(n.bit_length(), 33):
        (got, pk), = _run_tensors(eng, [layers], ks, [res], bits=bits)
        _assert_same(got, want[0], ("pack, tensors", bits))
        assert np.array_equal(pk, sr.packed_ref(locs[0], bits)), ("tensors", bits)
        got = _run_tensors(eng, [layers, layers2], ks, [res, res2], bits=bits, cohort=True)
        for c in range(2):
            _assert_same(got[c][0], want[c], ("pack, cohort", bits, c))
            assert np.array_equal(got[c][1], sr.packed_ref(locs[c], bits)), ("cohort", bits, c)


def test_packed_ref_is_to_big_int_on_the_device():
    from flashe_amd import weights as wz
    rng = np.random.Generator(np.random.PCG64(9))
    for bits, K in ((12, 64), (13, 37), (25, 1), (32, 5)):
        loc = np.sort(rng.choice(1 << min(bits, 20), K, replace=False)).astype(np.uint32)
        big, le = wz.to_big_int(loc.astype(np.uint64), bits)
        assert le == K and big == int.from_bytes(sr.packed_ref(loc, bits).tobytes(), "little")


# ---------------------------------------------------------------------------------------------------------------- e. k == 0
def _sum(x, r):
    with np.errstate(over="ignore"):                                            # (max + max = inf is among the inputs)
        return x + r


def _k0_layers(kind):
    return [sr.build_pool(kind, n, 300 + n)[:2] for n in (1, 5, 1024, 1025, 4097)]


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_a_layer_that_keeps_nothing_only_updates_its_residual(E, eng, kind):
    """k == 0 pinned: residual <- x + residual, nothing written to loc / vals, FLASHE_OK -- for one layer, for every layer of a batch and for
    some of them, through every entry point, with a residual and with NULL, with loc / vals present and (where nothing at all is kept)
    NULL."""
    pairs = _k0_layers(kind)
    dt = pairs[0][0].dtype
    for l, r in pairs:                                                          # one layer
        loc, vals, new = eng.sparsify(l, 0, r)
        assert loc.size == 0 and vals.size == 0 and new.tobytes() == _sum(l, r).tobytes()
        loc, vals, new = eng.sparsify(l, 0, None)
        assert loc.size == 0 and vals.size == 0 and new is None
        dx, dl, dv = eng.upload(l), eng.upload(np.full(64, SENT, np.uint8)), eng.upload(np.full(64, SENT, np.uint8))
        for with_out in (True, False):
            dr = eng.upload(r)
            eng.sparsify_dev(l.size, 0, dx, dt == np.float64, dr, dl if with_out else None, dv if with_out else None)
            assert dr.download(dt, l.size).tobytes() == _sum(l, r).tobytes()
            eng.sparsify_dev(l.size, 0, dx, dt == np.float64, None, dl if with_out else None, dv if with_out else None)
        assert (dl.download(np.uint8) == SENT).all() and (dv.download(np.uint8) == SENT).all()
        with pytest.raises(E.FlasheError):
            eng.sparsify_dev(l.size, 1, dx, dt == np.float64, None, None, dv)              # something is kept: loc must be there
    for ks in ([0] * len(pairs), [0, 2, 0, 1025, 0], [1, 0, 512, 0, 4097]):     # every layer of a batch / some of them
        cases = [(l, r, k) for (l, r), k in zip(pairs, ks)]
        res = [r for _l, r in pairs]
        want = [sr.topk_ref(l, k, r) for l, r, k in cases]
        want0 = [sr.topk_ref(l, k, None) for l, _r, k in cases]
        for (l, r, k), w in zip(cases, want):
            assert k or (w[0].size == 0 and w[2].tobytes() == _sum(l, r).tobytes())
        _assert_same(_run_batch(eng, cases, res), want, ("k == 0, batch", kind, ks))
        _assert_same(_run_batch(eng, cases, None), want0, ("k == 0, batch, NULL residual", kind, ks))
        _assert_same(_run_batch_dev(eng, cases, res), want, ("k == 0, batch_dev", kind, ks))
        _assert_same(_run_batch_dev(eng, cases, None), want0, ("k == 0, batch_dev, NULL residual", kind, ks))
        ns = [l.size for l, _r in pairs]
        layers = [l for l, _r in pairs]
        (got, _pk), = _run_tensors(eng, [layers], ks, [res], bits=14)
        _assert_same(got, _model_wide(want, ns), ("k == 0, tensors", kind, ks))
        (got, _pk), = _run_tensors(eng, [layers], ks, None, bits=14)
        _assert_same(got, _model_wide(want0, ns), ("k == 0, tensors, NULL residual", kind, ks))
        got = _run_tensors(eng, [layers, layers[:]], ks, [res, [w[2] for w in want]], bits=14, cohort=True)
        _assert_same(got[0][0], _model_wide(want, ns), ("k == 0, cohort", kind, ks))
        _assert_same(got[1][0], _model_wide([sr.topk_ref(l, k, w[2]) for (l, _r, k), w in zip(cases, want)], ns), ("k == 0, cohort, client 1", kind, ks))
        got = _run_tensors(eng, [layers, layers[:]], ks, None, bits=14, cohort=True)
        _assert_same(got[0][0], _model_wide(want0, ns), ("k == 0, cohort, NULL residual", kind, ks))
    # nothing kept in the whole call: the residual alone is written, and loc / vals may be NULL
    flat, rflat = np.concatenate([l for l, _r in pairs]), np.concatenate([r for _l, r in pairs])
    dx, dr = eng.upload(flat), eng.upload(rflat)
    eng.sparsify_batch_dev([l.size for l, _r in pairs], [0] * len(pairs), dx, dt == np.float64, dr, None, None)
    assert dr.download(dt, flat.size).tobytes() == _sum(flat, rflat).tobytes()
    eng.sparsify_batch_dev([l.size for l, _r in pairs], [0] * len(pairs), dx, dt == np.float64, None, None, None)
    codes = _codes()
    starts = np.concatenate([[0], np.cumsum([l.size for l, _r in pairs])[:-1]])
    dr = eng.upload(rflat)
    table = [(int(s), dx.ptr + int(s) * dt.itemsize, codes[kind]) for s in starts]
    eng.sparsify_tensors_dev(flat.size, table, [0] * len(pairs), dr, None, None)
    assert dr.download(dt, flat.size).tobytes() == _sum(flat, rflat).tobytes()
    with pytest.raises(E.FlasheError):
        eng.sparsify_tensors_dev(flat.size, table, [0, 1, 0, 0, 0], dr, None, None)
