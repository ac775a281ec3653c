"""GPU: every kernel site of the quantise / batch codec against the independent reference of tests/codec_ref.py over the edge plane
(+-0, +-alpha and their neighbours, +-inf, subnormals, the dtype's extremes, values whose scaled image is an integer or an ulp off it,
draws of exactly 0 and 1 - 2^-53, widths 1..62), bit for bit.  Where a cipher sits between the codec and the result, the expected
value is the reference's codec composed with the oracle's cipher.  Equality is the contract: no tolerance anywhere."""
import numpy as np
import pytest

import codec_ref as R

pytestmark = pytest.mark.gpu

KEY = bytes(range(32))
FUSED_ALPHAS = (8.17121, 3e-3, 1e-30, 1e30)


@pytest.fixture(scope="module")
def E():
    from flashe_amd import engine
    return engine


def _eq_q(got, want, *what):
    got, want = np.asarray(got, dtype=np.uint64).reshape(-1), np.asarray(want).astype(np.uint64).reshape(-1)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad[:4], got[bad[:4]], want[bad[:4]], bad.size)


def _eq_f(got, want, *what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert got.tobytes() == want.tobytes(), (what, bad[:4], got[bad[:4]], want[bad[:4]], bad.size)


def _limbs(q, L):
    out = np.zeros((len(q), L), dtype=np.uint64)
    out[:, 0] = np.asarray(q).astype(np.uint64)
    return out


_bits16 = R.bits16


# ------------------------------------------------------------------------------------------------ plain quantise / unquantise
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_plain_quantize_device_and_host_twin(E, dtype):
    eng = E.Engine(KEY, 64, device=0)
    kept, _ = R.quantize_cases(dtype)
    assert len(kept) >= (77 if dtype == np.float32 else 84)
    for alpha in R.ALPHAS:
        x = R.edge_plane(dtype, alpha)
        n = len(x)
        dx, dq = eng.upload(x), eng.alloc(8 * n)
        for kind in R.DRAWS:
            u = R.draws(kind, n)
            du = eng.upload(u)
            for bits in [w for a, w in kept if a == alpha]:
                want = R.ref_quantize(x, alpha, bits, u)
                eng.quantize_dev(n, dx, dtype == np.float64, alpha, bits, du, dq)
                got = dq.download(np.uint64, n)
                _eq_q(got, want, "quantize_dev", dtype.__name__, alpha, bits, kind)
                R.check_properties(x, alpha, bits, got, u)
                _eq_q(eng.quantize(x, alpha, bits, u), want, "quantize (host twin)", dtype.__name__, alpha, bits, kind)


@pytest.mark.parametrize("bits,C", R.PAIRS)
def test_plain_unquantize_one_and_two_limbs(E, bits, C):
    eng = {1: E.Engine(KEY, 64, device=0), 2: E.Engine(KEY, 128, device=0)}
    for alpha in (6.5, 8.17121, 1e-30):
        for limbs in (1, 2):
            vals = R.sum_plane(bits, C, int_bits=64 * limbs)
            if (bits, C) == (62, 5) and limbs == 2:
                vals.append(0x13ffffffffffffffb)
            want = R.ref_unquantize(vals, alpha, bits, C)
            v = R.to_limbs(vals, limbs)
            n = len(vals)
            dv, dout = eng[limbs].upload(v), eng[limbs].alloc(8 * n)
            eng[limbs].unquantize_dev(n, dv, limbs, alpha, bits, C, dout)
            _eq_f(dout.download(np.float64, n), want, "unquantize_dev", bits, C, alpha, limbs)
            _eq_f(eng[limbs].unquantize(v, alpha, bits, C), want, "unquantize (host twin)", bits, C, alpha, limbs)


# ------------------------------------------------------------------------------------------------ fused with the cipher
def _agg_that_decrypts_to(oracle, vals, it, add_idx, minus_idx, J, b):
    """The aggregate whose decrypt is `vals` (Python ints below 2^b)."""
    L = 2 if b > 64 else 1
    P = R.to_limbs(vals, L)
    d0 = oracle.decrypt(KEY, it, add_idx, minus_idx, J, b, np.zeros_like(P))
    agg = oracle.combine(b, P, minus=d0)
    assert R.from_limbs(oracle.decrypt(KEY, it, add_idx, minus_idx, J, b, agg)) == [int(v) for v in vals]
    return agg


@pytest.mark.parametrize("chain", [1, 0])
@pytest.mark.parametrize("b,scheme", [(20, "single"), (20, "double"), (64, "single"), (64, "double"), (128, "single"), (128, "double")])
def test_fused_quantize_encrypt_and_decrypt_unquantize(E, oracle, monkeypatch, b, scheme, chain):
    monkeypatch.setenv("FLASHE_CHAIN", str(chain))                    # read when the engine is created
    eng = E.Engine(KEY, b, device=0)
    L, J, it, idx = (2 if b > 64 else 1), 7, 5, 3
    sch = E.SCHEME_DOUBLE if scheme == "double" else E.SCHEME_SINGLE
    widths = [w for w in R.FUSED_WIDTHS if w <= b]
    n_cases = 0
    for dtype in (np.float32, np.float64):
        for alpha in FUSED_ALPHAS:
            x, u = R.crossed_plane(dtype, alpha)
            n = len(x)
            dx, du, dct = eng.upload(x), eng.upload(u), eng.alloc_vec(n)
            for bits in widths:
                if R.overflows(dtype, alpha, bits):
                    continue
                q = R.ref_quantize(x, alpha, bits, u)
                eng.quantize_encrypt_dev(it, idx, sch, n, J, dx, dtype == np.float64, alpha, bits, du, dct)
                ct = dct.download(np.uint64, n * L).reshape(n, L)
                want = oracle.encrypt(KEY, it, idx, scheme, J, b, _limbs(q, L))
                assert np.array_equal(ct, want), ("quantize_encrypt_dev", b, scheme, chain, dtype.__name__, alpha, bits,
                                                  np.flatnonzero((ct != want).any(axis=1))[:4])
                n_cases += 1
    assert n_cases >= (2 * 4 * len(widths) - 4)                       # float32 loses alpha = 1e30 at 32, 33, 53, 62 bits and nothing else
    for bits, C in ([(16, 10)] if b == 20 else [p for p in R.PAIRS if p[0] <= b]):
        vals = R.sum_plane(bits, C, int_bits=b)
        n = len(vals)
        for add_idx, minus_idx in [([C], [0]), ([], list(range(min(C, 40))))]:
            agg = _agg_that_decrypts_to(oracle, vals, it, add_idx, minus_idx, J, b)
            dagg, dout = eng.upload(agg), eng.alloc(8 * n)
            for alpha in (6.5, 1e-30):
                eng.decrypt_unquantize_dev(it, add_idx, minus_idx, n, J, dagg, alpha, bits, C, dout)
                _eq_f(dout.download(np.float64, n), R.ref_unquantize(vals, alpha, bits, C), "decrypt_unquantize_dev", b, chain, bits, C, alpha)


# ------------------------------------------------------------------------------------------------ model tables
MODEL = [(np.float32, 8.17121, 4001), (np.float64, 3e-3, 1), (np.float32, 1e-30, 2999), (np.float64, 1e30, 5000), (np.float32, 0.1, 3)]


def _model(eng, seed=0, model=MODEL):
    """layers (x, alpha, start), their device copies, the flat draws."""
    layers, at = [], 0
    for i, (dt, alpha, size) in enumerate(model):
        x = R.layer_fill(dt, alpha, size, seed + i)
        layers.append((x, alpha, at, eng.upload(x)))
        at += size
    return layers, at, R.mixed_draws(at, seed)


def _model_q(layers, bits, u):
    return np.concatenate([R.ref_quantize(x, alpha, bits, u[at:at + len(x)]) for x, alpha, at, _d in layers])


@pytest.mark.parametrize("b,scheme,bits", [(64, "double", 16), (64, "single", 33), (128, "double", 62), (20, "double", 16), (128, "single", 24)])
def test_model_tables_pick_each_layers_alpha_and_dtype(E, oracle, b, scheme, bits):
    eng = E.Engine(KEY, b, device=0)
    L, J, it, idx, C = (2 if b > 64 else 1), 5, 11, 2, 3
    sch = E.SCHEME_DOUBLE if scheme == "double" else E.SCHEME_SINGLE
    model = [m for m in MODEL if not R.overflows(m[0], m[1], bits)]
    assert len(model) == len(MODEL)
    layers, n, u = _model(eng)
    q = _model_q(layers, bits, u)
    want = oracle.encrypt(KEY, it, idx, scheme, J, b, _limbs(q, L))
    table = [(at, d.ptr, alpha, x.dtype == np.float64) for x, alpha, at, d in layers]
    du, dct = eng.upload(u), eng.alloc_vec(n)
    # windows: the whole model; one that starts inside layer 0 and ends inside layer 3; one value either side of a boundary
    for first, count in [(0, n), (1234, 9000), (4000, 2), (n - 1, 1), (4001, 1)]:
        eng.memset_dev(dct, 0xEE, 8 * L * n)
        eng.quantize_encrypt_model_dev(it, idx, sch, n, J, first, count, table, bits, E.DeviceBufferView(du, 8 * first, 8 * count),
                                       E.DeviceBufferView(dct, 8 * L * first, 8 * L * count))
        ct = dct.download(np.uint64, n * L).reshape(n, L)
        assert np.array_equal(ct[first:first + count], want[first:first + count]), ("quantize_encrypt_model_dev", b, bits, first, count)
        untouched = np.delete(ct, np.s_[first:first + count], axis=0)
        assert (untouched == np.uint64(0xEEEEEEEEEEEEEEEE)).all(), "wrote outside its window"
    # the way back: every layer's own alpha, with and without a decrypt in front
    vals = np.resize(np.array(R.sum_plane(min(bits, b - 2), C, int_bits=b), dtype=object), n).tolist()
    back = [(at, None, alpha, False) for _x, alpha, at, _d in layers]
    want_f = np.concatenate([R.ref_unquantize(vals[at:at + len(x)], alpha, bits, C) for x, alpha, at, _d in layers])
    agg = _agg_that_decrypts_to(oracle, vals, it, [C], [0], J, b)
    dagg, dpl, dout = eng.upload(agg), eng.upload(R.to_limbs(vals, L)), eng.alloc(8 * n)
    for first, count in [(0, n), (1234, 9000), (4000, 2)]:
        eng.decrypt_unquantize_model_dev(it, [C], [0], n, J, first, count, E.DeviceBufferView(dagg, 8 * L * first, 8 * L * count), back, bits, C, dout)
        _eq_f(dout.download(np.float64, count), want_f[first:first + count], "decrypt_unquantize_model_dev", b, bits, first)
        eng.unquantize_model_dev(n, first, count, E.DeviceBufferView(dpl, 8 * L * first, 8 * L * count), back, bits, C, dout)
        _eq_f(dout.download(np.float64, count), want_f[first:first + count], "unquantize_model_dev", b, bits, first)
    for add, minus in [(None, None), (agg, None), (agg, R.to_limbs(vals, L))]:
        inp = R.to_limbs(vals, L)
        eng.combine_unquantize_model_dev(n, eng.upload(inp), None if add is None else eng.upload(add), None if minus is None else eng.upload(minus),
                                         back, bits, C, dout)
        after = R.from_limbs(oracle.combine(b, inp, add, minus))
        want_c = np.concatenate([R.ref_unquantize(after[at:at + len(x)], alpha, bits, C) for x, alpha, at, _d in layers])
        _eq_f(dout.download(np.float64, n), want_c, "combine_unquantize_model_dev", b, bits)


# ------------------------------------------------------------------------------------------------ batched
# int_bits, field_bits, element_bits, C; the last two: field_bits == element_bits, where q == 2^bits carries into the neighbouring field
BATCHED = [(128, 20, 16, 10), (120, 20, 16, 10), (64, 17, 16, 2), (100, 33, 32, 2), (64, 64, 62, 4), (120, 24, 24, 1), (128, 25, 25, 1)]


def _batched_ref(layers, u, b, fb, eb):
    """The batched plaintext (Python ints) and the element count, every layer quantised and padded on its own."""
    out = []
    for x, alpha, at, _d in layers:
        out += R.ref_batch(R.ref_quantize(x, alpha, eb, u[at:at + len(x)]), b, fb)
    return out


@pytest.mark.parametrize("b,fb,eb,C", BATCHED)
def test_batched_model_both_ways(E, b, fb, eb, C):
    eng = E.Engine(KEY, b, device=0)
    L, bs = (2 if b > 64 else 1), b // fb
    layers, n, u = _model(eng, seed=fb)
    assert any(len(x) % bs for x, _a, _s, _d in layers) or bs == 1
    want = _batched_ref(layers, u, b, fb, eb)
    if eb == 32 or fb == eb:
        assert any((R.ref_quantize(x, a, eb, u[s:s + len(x)]) == 1 << eb).any() for x, a, s, _d in layers), "q == 2^bits inside a padded field"
    ne = len(want)
    table = [(len(x), d.ptr, alpha, x.dtype == np.float64) for x, alpha, _at, d in layers]
    du, dout = eng.upload(u), eng.alloc_vec(ne)
    eng.quantize_batch_model_dev(table, eb, fb, du, ne, dout)
    assert R.from_limbs(dout.download(np.uint64, ne * L).reshape(ne, L)) == want, ("quantize_batch_model_dev", b, fb)
    # the way back: fields that hold sums of C uploads, the top of the field included
    plane = [v for v in R.sum_plane(eb, C, int_bits=min(fb, 64))]
    items, want_f = [], []
    for i, (x, alpha, _at, _d) in enumerate(layers):
        vals = np.resize(np.array(plane[i:] + [(1 << fb) - 1], dtype=object), len(x)).tolist()
        items += R.ref_batch(vals, b, fb)
        assert R.ref_unbatch(R.ref_batch(vals, b, fb), b, fb)[:len(vals)] == vals
        want_f.append(R.ref_unquantize(vals, alpha, eb, C))
    assert len(items) == ne
    dfl = eng.alloc(8 * n)
    eng.unbatch_unquantize_model_dev([(len(x), None, alpha, False) for x, alpha, _at, _d in layers], eb, fb, C, eng.upload(R.to_limbs(items, L)), ne, dfl)
    _eq_f(dfl.download(np.float64, n), np.concatenate(want_f), "unbatch_unquantize_model_dev", b, fb)


# ------------------------------------------------------------------------------------------------ precompute combine forms
@pytest.mark.parametrize("b,scheme,bits", [(128, "double", 62), (128, "single", 16), (64, "double", 33), (64, "single", 16), (20, "double", 16)])
def test_prepared_model_forms(E, oracle, b, scheme, bits):
    eng = E.Engine(KEY, b, device=0)
    L, J, it, idx, C = (2 if b > 64 else 1), 6, 21, 1, 4
    sch = E.SCHEME_DOUBLE if scheme == "double" else E.SCHEME_SINGLE
    layers, n, u = _model(eng, seed=b)
    du = eng.upload(u)
    q = _model_q(layers, bits, u)
    table = [(at, d.ptr, alpha, x.dtype == np.float64) for x, alpha, at, d in layers]
    # un-batched, in two range calls (the one that ends at n consumes the cache)
    eng.prepare_encrypt(it, idx, sch, n, J)
    add, minus = eng.prepared_download(eng.PREPARED_ENCRYPT, "add"), eng.prepared_download(eng.PREPARED_ENCRYPT, "minus")
    assert add is not None and (minus is not None) == (scheme == "double")
    dct = eng.alloc_vec(n)
    for first, count in [(0, 4321), (4321, n - 4321)]:
        eng.quantize_encrypt_prepared_model_dev(n, first, count, table, bits, E.DeviceBufferView(du, 8 * first, 8 * count),
                                                E.DeviceBufferView(dct, 8 * L * first, 8 * L * count))
    want = oracle.combine(b, _limbs(q, L), add, minus)
    assert np.array_equal(dct.download(np.uint64, n * L).reshape(n, L), want), ("quantize_encrypt_prepared_model_dev", b, scheme, bits)
    # batched
    fb = bits + 2
    if fb <= b:
        batched = _batched_ref(layers, u, b, fb, bits)
        ne = len(batched)
        eng.prepare_encrypt(it, idx, sch, ne, J)
        add, minus = eng.prepared_download(eng.PREPARED_ENCRYPT, "add"), eng.prepared_download(eng.PREPARED_ENCRYPT, "minus")
        dct = eng.alloc_vec(ne)
        eng.quantize_batch_encrypt_prepared_model_dev([(len(x), d.ptr, alpha, x.dtype == np.float64) for x, alpha, _at, d in layers], bits, fb, du, ne, dct)
        want = oracle.combine(b, R.to_limbs(batched, L), add, minus)
        assert np.array_equal(dct.download(np.uint64, ne * L).reshape(ne, L), want), ("quantize_batch_encrypt_prepared_model_dev", b, scheme, bits)
    # the way back from the prepared decrypt masks
    vals = np.resize(np.array(R.sum_plane(min(bits, b - 2), C, int_bits=b), dtype=object), n).tolist()
    back = [(at, None, alpha, False) for _x, alpha, at, _d in layers]
    want_f = np.concatenate([R.ref_unquantize(vals[at:at + len(x)], alpha, bits, C) for x, alpha, at, _d in layers])
    eng.prepare_decrypt(it, C, n, J)
    add, minus = eng.prepared_download(eng.PREPARED_DECRYPT, "add"), eng.prepared_download(eng.PREPARED_DECRYPT, "minus")
    inp = oracle.combine(b, oracle.combine(b, R.to_limbs(vals, L), minus=add), add=minus)      # (inp + add - minus) mod 2^b == vals
    dout = eng.alloc(8 * n)
    eng.decrypt_prepared_unquantize_model_dev(it, [], [], n, J, eng.upload(inp), back, bits, C, dout)
    _eq_f(dout.download(np.float64, n), want_f, "decrypt_prepared_unquantize_model_dev", b, bits)
    if fb <= b:
        plane = R.sum_plane(bits, C, int_bits=min(fb, 64))
        items, want_b = [], []
        for i, (x, alpha, _at, _d) in enumerate(layers):
            v = np.resize(np.array(plane[i:] + [(1 << fb) - 1], dtype=object), len(x)).tolist()
            items += R.ref_batch(v, b, fb)
            want_b.append(R.ref_unquantize(v, alpha, bits, C))
        ne = len(items)
        eng.prepare_decrypt(it, C, ne, J)
        add, minus = eng.prepared_download(eng.PREPARED_DECRYPT, "add"), eng.prepared_download(eng.PREPARED_DECRYPT, "minus")
        inp = oracle.combine(b, oracle.combine(b, R.to_limbs(items, L), minus=add), add=minus)
        eng.decrypt_prepared_unbatch_unquantize_model_dev(it, [], [], J, [(len(x), None, alpha, False) for x, alpha, _at, _d in layers], bits, fb, C,
                                                          eng.upload(inp), ne, dout)
        _eq_f(dout.download(np.float64, n), np.concatenate(want_b), "decrypt_prepared_unbatch_unquantize_model_dev", b, bits)


# ------------------------------------------------------------------------------------------------ tensors front end
try:
    # (asked at collection: once a test has created an engine, the framework of the same process no longer finds its device)
    import torch as _torch_mod
    _TORCH_GPU = _torch_mod.cuda.is_available()
except ImportError:
    _TORCH_GPU = False


def _torch():
    torch = pytest.importorskip("torch")
    if not (_TORCH_GPU and torch.cuda.is_available()):
        pytest.skip("no GPU visible to torch")
    return torch


# storage, alpha, shift (None = off), wide, loop64, size
TENSOR_MODEL = [("float16", 8.17121, None, False, False, 3001), ("bfloat16", 3e-3, 0.001, False, False, 1), ("float32", 1e-30, None, False, False, 2000),
                ("float64", 1e30, -0.25, False, False, 2503), ("float32", 0.1, 0.0625, True, False, 1777), ("float16", 1.0, 0.3, True, True, 999),
                ("bfloat16", 8.17121, None, False, True, 1200), ("float32", 3e-3, 1e-4, False, True, 801), ("float32", 8.17121, 0.7, False, False, 1303)]


def _tensor_model(torch, eng, seed):
    """The torch tensors, their flashe_tensor_layer rows, and the reference's compute-type arrays (upcast, shifted, widened)."""
    from flashe_amd import _lib
    code = {"float32": _lib.TENSOR_F32, "float64": _lib.TENSOR_F64, "float16": _lib.TENSOR_F16, "bfloat16": _lib.TENSOR_BF16}
    tdt = {"float32": torch.float32, "float64": torch.float64, "float16": torch.float16, "bfloat16": torch.bfloat16}
    rows, ref, keep, at = [], [], [], 0
    for i, (storage, alpha, shift, wide, loop64, size) in enumerate(TENSOR_MODEL):
        base = np.float64 if storage == "float64" else np.float32
        x = R.layer_fill(base, alpha, size, seed + i, storage=storage if storage in ("float16", "bfloat16") else None)
        t = torch.from_numpy(x).to(tdt[storage]).to("cuda:0")
        if storage in ("float16", "bfloat16"):
            assert np.array_equal(R.upcast16(t.cpu() if storage == "bfloat16" else t.cpu().numpy()), x, equal_nan=False), storage
        flags = 0
        if shift is not None:
            flags |= _lib.TENSOR_SHIFT | (_lib.TENSOR_SHIFT_WIDE if wide else 0)
            x = R.ref_shift(x, np.float64(shift) if wide else float(shift))
        if loop64:
            flags |= _lib.TENSOR_LOOP_F64
            x = x.astype(np.float64)
        fa = eng.foreign(t, what=f"layer {i}")
        keep.append((t, fa))
        rows.append((at, fa.ptr, alpha, 0.0 if shift is None else shift, code[storage], flags))
        ref.append((x, alpha, at, None))
        at += size
    torch.cuda.synchronize()
    return rows, ref, keep, at


@pytest.mark.parametrize("b,scheme,bits", [(128, "double", 16), (64, "single", 24), (64, "double", 53)])
def test_tensor_front_end_upcasts_shifts_and_widens_like_numpy(E, oracle, b, scheme, bits):
    torch = _torch()
    eng = E.Engine(KEY, b, device=0)
    L, J, it, idx = (2 if b > 64 else 1), 5, 8, 2
    sch = E.SCHEME_DOUBLE if scheme == "double" else E.SCHEME_SINGLE
    rows, ref, keep, n = _tensor_model(torch, eng, seed=bits)
    assert all(not R.overflows(x.dtype, alpha, bits) for x, alpha, _at, _d in ref)
    u = R.mixed_draws(n, bits)
    q = _model_q(ref, bits, u)
    du, dct = eng.upload(u), eng.alloc_vec(n)
    want = oracle.encrypt(KEY, it, idx, scheme, J, b, _limbs(q, L))
    for first, count in [(0, n), (2999, 3000)]:
        eng.quantize_encrypt_tensors_dev(it, idx, sch, n, J, first, count, rows, bits, E.DeviceBufferView(du, 8 * first, 8 * count),
                                         E.DeviceBufferView(dct, 8 * L * first, 8 * L * count))
        ct = dct.download(np.uint64, n * L).reshape(n, L)[first:first + count]
        bad = np.flatnonzero((ct != want[first:first + count]).any(axis=1))
        assert bad.size == 0, ("quantize_encrypt_tensors_dev", b, bits, first, bad[:4] + first)
    fb = bits + 1
    if fb <= b:
        batched = _batched_ref(ref, u, b, fb, bits)
        ne = len(batched)
        dout = eng.alloc_vec(ne)
        eng.quantize_batch_tensors_dev(rows, n, bits, fb, du, ne, dout)
        assert R.from_limbs(dout.download(np.uint64, ne * L).reshape(ne, L)) == batched, ("quantize_batch_tensors_dev", b, bits)
    eng.sync()
    del keep


# ------------------------------------------------------------------------------------------------ cohort chain
def test_cohort_chain_quantises_from_raw_bits_like_numpy(E, oracle):
    """One chained launch for two clients: rows of both compute types with odd sizes (so that the two-element groups of the chain
    straddle row boundaries and take the per-lane form), long uniform rows (the fast path), an edge value either side of every
    boundary, a float16 source and a float32 source under a float64 row (both staged)."""
    from flashe_amd import _lib
    b, bits, it, J, C = 128, 24, 4, 16, 2
    eng = E.Engine(KEY, b, device=0)
    need = 2 * eng.cu_count * 16 * 256
    sizes = [need // 2 + 1, 3, 1, need // 4 + 7, 0]
    sizes[-1] = need + 513 - sum(sizes)
    n = sum(sizes)
    spec = [(np.float32, 8.17121, 0), (np.float64, 3e-3, 0), (np.float32, 1e-30, 0), (np.float32, 0.1, 0), (np.float32, 1.0, _lib.TENSOR_LOOP_F64)]
    rows, starts, at = [], [], 0
    for (dt, alpha, flags), size in zip(spec, sizes):
        rows.append((at, None, alpha, 0.0, _lib.TENSOR_F64 if dt == np.float64 else _lib.TENSOR_F32, flags))
        starts.append(at)
        at += size
    u = R.mixed_draws(C * n, 3)
    srcs, dts, want, keep = [], [], [], []
    for c in range(C):
        srow, drow, q = [], [], []
        for li, ((dt, alpha, flags), size) in enumerate(zip(spec, sizes)):
            half = c == 1 and li == 3
            x = R.layer_fill(dt, alpha, size, seed=10 * c + li, storage="float16" if half else None)
            d = eng.upload(_bits16(x, "float16") if half else x)
            keep.append(d)
            srow.append(d.ptr)
            drow.append(_lib.TENSOR_F16 if half else (_lib.TENSOR_F64 if dt == np.float64 else _lib.TENSOR_F32))
            xr = x.astype(np.float64) if flags & _lib.TENSOR_LOOP_F64 else x
            q.append(R.ref_quantize(xr, alpha, bits, u[c * n + starts[li]:c * n + starts[li] + size]))
        srcs.append(srow)
        dts.append(drow)
        want.append(oracle.encrypt(KEY, it, 5 + c, "double", J, b, _limbs(np.concatenate(q), 2)))
    cts, dsum = [eng.alloc_vec(n) for _ in range(C)], eng.alloc_vec(n)
    assert eng.quantize_encrypt_cohort_dev(it, 5, n, J, rows, srcs, dts, bits, eng.upload(u), cts, dsum), "the chained cohort launch declined the shape"
    for c in range(C):
        got = cts[c].download(np.uint64, 2 * n).reshape(n, 2)
        bad = np.flatnonzero((got != want[c]).any(axis=1))
        assert bad.size == 0, ("quantize_encrypt_cohort_dev", c, bad[:6], [int(np.searchsorted(starts, i, side="right") - 1) for i in bad[:6]])
    assert np.array_equal(dsum.download(np.uint64, 2 * n).reshape(n, 2), oracle.aggregate_elem(want, b))


# ------------------------------------------------------------------------------------------------ sparse cohort front end
@pytest.mark.parametrize("bits,zzz_is_f64,odd", [(16, False, 0), (32, True, 1), (62, False, 1), (24, True, 0)])
def test_sparse_cohort_front_end(E, bits, zzz_is_f64, odd):
    """flashe_quantize_cohort_dev: rows that end inside a 1024-value tile, edge values at row and tile ends, and (odd = 1) sources,
    draws and plaintexts at addresses that are not 16-byte aligned, which takes the scalar form of every vector access.  The trailing
    'zzz' value (alpha 1.0) at +-1.0 and beyond."""
    from flashe_amd import _lib
    eng = E.Engine(KEY, 64, device=0)
    # storage, alpha, shift, wide, loop64, size
    spec = [("float32", 8.17121, None, False, False, 2048 + 1024 + 5), ("float16", 3e-3, None, False, False, 1019), ("float64", 8.17121, -0.5, False, False, 2050),
            ("float32", 1e-30, None, False, True, 1024), ("bfloat16", 1.0, 0.25, True, False, 3), ("float32", 0.1, 0.01, False, False, 4099)]
    spec = [s for s in spec if not R.overflows(np.float64 if s[0] == "float64" or s[4] else np.float32, s[1], bits)]
    assert len(spec) == 6
    code = {"float32": _lib.TENSOR_F32, "float64": _lib.TENSOR_F64, "float16": _lib.TENSOR_F16, "bfloat16": _lib.TENSOR_BF16}
    zzz = [1.0, -1.0, 2.5, -7.0, 0.0, float(np.nextafter(np.float32(1), np.float32(0)))]
    C, n = len(zzz), sum(s[5] for s in spec)
    stride = n + 1 + odd
    u = R.mixed_draws(C * stride + odd, bits)
    rows, at = [], 0
    for storage, alpha, shift, wide, loop64, size in spec:
        flags = (_lib.TENSOR_SHIFT if shift is not None else 0) | (_lib.TENSOR_SHIFT_WIDE if wide else 0) | (_lib.TENSOR_LOOP_F64 if loop64 else 0)
        rows.append((at, None, alpha, 0.0 if shift is None else shift, _lib.TENSOR_F64 if storage == "float64" else _lib.TENSOR_F32, flags))
        at += size
    srcs, dts, want, keep = [], [], [], []
    for c in range(C):
        srow, drow, q, at = [], [], [], 0
        for li, (storage, alpha, shift, wide, loop64, size) in enumerate(spec):
            half = storage in ("float16", "bfloat16")
            x = R.layer_fill(np.float64 if storage == "float64" else np.float32, alpha, size, seed=7 * c + li, storage=storage if half else None)
            for tile_end in range(1024 - at % 1024, size, 1024):            # an edge value either side of every tile end
                x[tile_end - 1], x[tile_end] = (np.inf, -np.inf) if half else (x.dtype.type(alpha), np.nextafter(-x.dtype.type(alpha), x.dtype.type(0)))
            raw = _bits16(x, storage) if half else x
            pad = odd * (8 if storage == "float64" else 4 if storage == "float32" else 2)
            d = eng.alloc(raw.nbytes + 16)
            d.upload_at(pad, raw)
            keep.append(d)
            srow.append(d.ptr + pad)
            drow.append(code[storage])
            if shift is not None:
                x = R.ref_shift(x, np.float64(shift) if wide else float(shift))
            if loop64:
                x = x.astype(np.float64)
            q.append(R.ref_quantize(x, alpha, bits, u[odd + c * stride + at:odd + c * stride + at + size]))
            at += size
        srcs.append(srow)
        dts.append(drow)
        zt = np.float64 if zzz_is_f64 else np.float32
        q.append(R.ref_quantize(np.array([zzz[c]], dtype=zt), 1.0, bits, u[odd + c * stride + n:odd + c * stride + n + 1]))
        want.append(np.concatenate(q))
    du = eng.upload(u)
    dpt = [eng.alloc(8 * (n + 2)) for _ in range(C)]
    dtail = [eng.alloc(16) for _ in range(C)]
    for d in dtail:
        eng.memset_dev(d, 0xEE, 16)
    dzero = eng.alloc(8 * C)
    eng.quantize_cohort_dev(n, rows, srcs, dts, bits, E.DeviceBufferView(du, 8 * odd, 8 * C * stride), stride, zzz, zzz_is_f64,
                            [E.DeviceBufferView(d, 8 * odd, 8 * n) for d in dpt], dtail, dzero)
    zeros = dzero.download(np.uint64, C)
    for c in range(C):
        _eq_q(dpt[c].download_at(8 * odd, np.uint64, n), want[c][:n], "quantize_cohort_dev", bits, odd, c)
        assert int(zeros[c]) == int(want[c][n]), ("zzz", bits, zzz_is_f64, zzz[c], int(zeros[c]), int(want[c][n]))
        t = dtail[c].download(np.uint64, 2)
        assert int(t[0]) == int(want[c][n]) and int(t[1]) == 0xEEEEEEEEEEEEEEEE, "the tail is one limb wide at int_bits = 64"
    # the properties the zzz values imply: +-1.0 and beyond clip to the ends of the range
    R.check_properties(np.array(zzz, dtype=np.float64 if zzz_is_f64 else np.float32), 1.0, bits, zeros, [u[odd + c * stride + n] for c in range(C)])
