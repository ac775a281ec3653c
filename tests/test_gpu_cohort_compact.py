"""GPU: a cohort's chained launch from the floats at int_bits <= 32 in the compact layout (flashe_quantize_encrypt_cohort_u32_dev,
prf_small_cohort_kernel; FlasheCohort(compact=True)).  ABI level on two CUs, where the launch admits a few tens of thousands of values:
every uint32 ciphertext against the fused client step of that client in the one-limb layout on the same engine, the sum against the
mod-2^b sum of them.  Class level at the chip's own admission length against sequential FlasheClients (the path tests/golden/
clientstep.json pins), everything compared as bytes or values and `up.path` asserted everywhere."""
import numpy as np
import pytest

from test_gpu_cohort import KEY, _W, _args, _host_models, _poison, _same_state, _sequential

pytestmark = pytest.mark.gpu

WIDTHS = [(16, 12), (20, 16), (23, 16), (24, 16), (32, 24)]            # int_bits, element_bits


@pytest.fixture(scope="module")
def E():
    from flashe_amd import engine
    return engine


def _length(b, J, cus=2, extra=0):
    """A length at or past the launch's admission on `cus` CUs whose chunks (d + 1 and d elements, both kinds present where J > 1) are no
    multiples of m: every chunk ends in a partial block, the tiles around the chunk ends walk, the last tile is partial."""
    from flashe_amd.block import compact_cohort_admission_length
    m, n = 128 // b, compact_cohort_admission_length(cus, b, J) + extra
    while (J > 1 and n % J == 0) or (n // J) % m == 0 or (n // J + 1) % m == 0:
        n += 1
    return n


def _sizes(n):
    head = [1, 7, 0, 10007, 256 * 37 + 91]
    return head + [n - sum(head)]


def _values(dtype, alpha, size, seed):
    """Values inside the clip range with the edges strewn in: beyond +-alpha, exactly +-alpha, 0."""
    g = np.random.Generator(np.random.PCG64(seed))
    x = (g.standard_normal(size) * alpha / 2).astype(dtype)
    for k, v in enumerate((alpha, -alpha, 0.0, 3 * alpha, -3 * alpha, np.nextafter(dtype(alpha), dtype(0)))):
        x[k::89] = v
    return x


def _cohort_case(E, eng, b, bits, J, C, n, it=3, first_idx=5, alias=False):
    """The shared rows, every client's sources and draws, and the per-client reference: quantize_encrypt_model_dev in the one-limb layout
    on the same engine with the same draws."""
    from flashe_amd import _lib
    sizes = _sizes(n)
    alphas = [0.37, 2.5, 1.0, 8.17121, 3e-3, 0.05]
    rows, starts, at = [], [], 0
    for li, size in enumerate(sizes):
        rows.append((at, None, alphas[li], 0.0, _lib.TENSOR_F64 if li % 2 else _lib.TENSOR_F32, 0))
        starts.append(at)
        at += size
    u = np.random.Generator(np.random.PCG64(b * 1000 + J * 10 + C)).random(C * n)
    u[::5] = 0.0
    u[1::5] = 1.0 - 2.0 ** -53
    du = eng.upload(u)
    srcs, dts, keep, want = [], [], [], []
    for c in range(C):
        if alias and c:
            srcs.append(srcs[0])
            dts.append(dts[0])
        else:
            xs = [_values(np.float64 if li % 2 else np.float32, alphas[li], size, 100 * c + li) for li, size in enumerate(sizes)]
            ds = [eng.upload(x) for x in xs]
            keep += ds
            srcs.append([d.ptr for d in ds])
            dts.append([_lib.TENSOR_F64 if li % 2 else _lib.TENSOR_F32 for li in range(len(sizes))])
        table = [(starts[li], srcs[c][li], alphas[li], bool(li % 2)) for li, size in enumerate(sizes) if size]
        ref = eng.alloc_vec(n)
        eng.quantize_encrypt_model_dev(it, first_idx + c, E.SCHEME_DOUBLE, n, J, 0, n, table, bits, E.DeviceBufferView(du, 8 * c * n, 8 * n), ref)
        want.append(ref.download(np.uint64, n).copy())
    return rows, srcs, dts, du, want, keep


def _run(E, eng, b, bits, J, C, n, alias=False, it=3, first_idx=5):
    rows, srcs, dts, du, want, keep = _cohort_case(E, eng, b, bits, J, C, n, it, first_idx, alias)
    cts, dsum = [eng.alloc(4 * n) for _ in range(C)], eng.alloc(4 * n)
    for d in cts + [dsum]:
        eng.memset_dev(d, 0xA5, 4 * n)
    ok = eng.quantize_encrypt_cohort_u32_dev(it, first_idx, n, J, rows, srcs, dts, bits, du, cts, dsum)
    got = [d.download(np.uint32, n).copy() for d in cts]
    gsum = dsum.download(np.uint32, n).copy()
    del keep
    return ok, got, gsum, want


def _check(got, gsum, want, b, *what):
    total = np.zeros(len(gsum), dtype=np.uint64)
    for c, (g, w) in enumerate(zip(got, want)):
        bad = np.flatnonzero(g.astype(np.uint64) != w)
        assert bad.size == 0, (what, "client", c, bad[:6], g[bad[:6]], w[bad[:6]], bad.size)
        total += w
    total &= np.uint64((1 << b) - 1)
    bad = np.flatnonzero(gsum.astype(np.uint64) != total)
    assert bad.size == 0, (what, "sum", bad[:6], gsum[bad[:6]], total[bad[:6]], bad.size)


# ------------------------------------------------------------------------------------------------ ABI level, two CUs
@pytest.mark.parametrize("J,C", [(16, 2), (7, 10), (1, 1)])
@pytest.mark.parametrize("b,bits", WIDTHS)
def test_the_compact_launch_is_every_clients_fused_step(E, b, bits, J, C):
    eng = E.Engine(KEY, b, device=0)
    eng.set_cu_limit(2)
    n = _length(b, J, extra=777)
    ok, got, gsum, want = _run(E, eng, b, bits, J, C, n)
    assert ok, "the chained compact cohort launch declined the shape"
    _check(got, gsum, want, b, b, J, C, n)


@pytest.mark.parametrize("J,C", [(16, 10), (7, 1), (1, 2), (16, 1)])
def test_the_shipped_width_at_the_other_chain_lengths(E, J, C):
    """int_bits 20 at C = 1 (two streams: the second counter shortcut) and 10 under the other chunkings."""
    eng = E.Engine(KEY, 20, device=0)
    eng.set_cu_limit(2)
    n = _length(20, J)
    ok, got, gsum, want = _run(E, eng, 20, 16, J, C, n)
    assert ok
    _check(got, gsum, want, 20, J, C, n)


@pytest.mark.parametrize("C", [128, 129])
def test_the_link_table_boundary(E, C):
    """kMaxLinks clients chain; one more is FLASHE_ENOTSUP with the outputs untouched.  Every client reads client 0's model."""
    eng = E.Engine(KEY, 20, device=0)
    eng.set_cu_limit(2)
    n = _length(20, 16)
    ok, got, gsum, want = _run(E, eng, 20, 16, 16, C, n, alias=True)
    if C == 128:
        assert ok
        _check(got, gsum, want, 20, C)
    else:
        assert ok is False
        assert all((g == np.uint32(0xA5A5A5A5)).all() for g in got + [gsum])


def test_the_last_prefix_is_refused(E):
    """first_idx + C - 1 = 2^32 - 1: the double mask's idx + 1 does not fit the prefix field."""
    eng = E.Engine(KEY, 20, device=0)
    eng.set_cu_limit(2)
    n = _length(20, 16)
    with pytest.raises(E.FlasheError) as ei:
        _run(E, eng, 20, 16, 16, 2, n, first_idx=2 ** 32 - 2)
    assert ei.value.code == -22
    ok, got, gsum, want = _run(E, eng, 20, 16, 16, 2, n, first_idx=2 ** 32 - 3)
    assert ok
    _check(got, gsum, want, 20, "top")


@pytest.mark.parametrize("b,bits", [(20, 16), (32, 24)])
def test_one_block_below_admission_is_declined_untouched(E, b, bits):
    from flashe_amd.block import compact_cohort_admission_length
    eng = E.Engine(KEY, b, device=0)
    eng.set_cu_limit(2)
    n = compact_cohort_admission_length(2, b, 16)
    ok, got, gsum, want = _run(E, eng, b, bits, 16, 3, n)
    assert ok
    _check(got, gsum, want, b, "at admission")
    ok, got, gsum, _want = _run(E, eng, b, bits, 16, 3, n - 1)
    assert ok is False
    assert all((g == np.uint32(0xA5A5A5A5)).all() for g in got + [gsum])


def test_a_ctx_without_the_compact_layout_declines(E):
    eng = E.Engine(KEY, 64, device=0)
    eng.set_cu_limit(2)
    assert not eng.compact_supported()
    n = _length(32, 16)
    x, u = eng.upload(np.zeros(n, np.float32)), eng.upload(np.zeros(n))
    ct, dsum = eng.alloc(4 * n), eng.alloc(4 * n)
    from flashe_amd import _lib
    assert eng.quantize_encrypt_cohort_u32_dev(0, 0, n, 16, [(0, None, 1.0, 0.0, _lib.TENSOR_F32, 0)], [[x.ptr]], [[_lib.TENSOR_F32]], 16, u, [ct], dsum) is False


def test_a_width_that_is_not_compiled_in_declines_untouched(E):
    """int_bits 21 has the compact layout but no chained cohort launch: FLASHE_ENOTSUP, nothing written."""
    eng = E.Engine(KEY, 21, device=0)
    eng.set_cu_limit(2)
    assert eng.compact_supported()
    ok, got, gsum, _want = _run(E, eng, 21, 16, 16, 2, _length(20, 16, extra=5000))
    assert ok is False
    assert all((g == np.uint32(0xA5A5A5A5)).all() for g in got + [gsum])


def test_staged_sources_float16_bfloat16_shift(E):
    """Sources that are not read in place take the one stage pass: float16 and bfloat16 storage, float32 under a float64 row, SHIFT.
    The reference is quantize_encrypt_tensors_dev of each client (which stages the same way) in the one-limb layout."""
    from flashe_amd import _lib
    b, bits, J, C, it = 20, 16, 16, 3, 9
    eng = E.Engine(KEY, b, device=0)
    eng.set_cu_limit(2)
    n = _length(b, J, extra=300)
    sizes = [4097, 3, n - 4100 - 9001, 9001]
    spec = [("float16", _lib.TENSOR_F32, 0, 0.0), ("bfloat16", _lib.TENSOR_F32, _lib.TENSOR_SHIFT, 0.0625),
            ("float32", _lib.TENSOR_F32, _lib.TENSOR_LOOP_F64, 0.0), ("float32", _lib.TENSOR_F32, _lib.TENSOR_SHIFT, -0.25)]
    codes = {"float16": _lib.TENSOR_F16, "bfloat16": _lib.TENSOR_BF16, "float32": _lib.TENSOR_F32}
    alpha = 1.5
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    rows = [(starts[li], None, alpha, sh, code, fl) for li, (_st, code, fl, sh) in enumerate(spec)]
    u = np.random.Generator(np.random.PCG64(5)).random(C * n)
    du = eng.upload(u)
    srcs, dts, keep, want = [], [], [], []
    for c in range(C):
        srow = []
        for li, ((st, _code, _fl, _sh), size) in enumerate(zip(spec, sizes)):
            x = _values(np.float32, alpha, size, 50 * c + li)
            if st == "float16":
                x = x.astype(np.float16).view(np.uint16)
            elif st == "bfloat16":
                x = (np.ascontiguousarray(x).view(np.uint32) >> np.uint32(16)).astype(np.uint16)
            d = eng.upload(x)
            keep.append(d)
            srow.append(d.ptr)
        srcs.append(srow)
        dts.append([codes[st] for st, _c, _f, _s in spec])
        trows = [(starts[li], srow[li], alpha, sh, codes[st], fl) for li, (st, _code, fl, sh) in enumerate(spec)]
        ref = eng.alloc_vec(n)
        eng.quantize_encrypt_tensors_dev(it, 1 + c, E.SCHEME_DOUBLE, n, J, 0, n, trows, bits, E.DeviceBufferView(du, 8 * c * n, 8 * n), ref)
        want.append(ref.download(np.uint64, n).copy())
    cts, dsum = [eng.alloc(4 * n) for _ in range(C)], eng.alloc(4 * n)
    assert eng.quantize_encrypt_cohort_u32_dev(it, 1, n, J, rows, srcs, dts, bits, du, cts, dsum)
    _check([d.download(np.uint32, n).copy() for d in cts], dsum.download(np.uint32, n).copy(), want, b, "staged")


# ------------------------------------------------------------------------------------------------ class level, the chip's admission length
def _cu_count():
    from flashe_amd import Engine
    return Engine(KEY, 20).cu_count


def _model_sizes(n):
    head = [1, 7, 0, 10007, 256 * 37 + 91]
    rest = n - sum(head)
    cuts = [rest // 7, rest // 3 + 5]
    return head + cuts + [rest - sum(cuts)]


def _values_of(dv):
    return np.asarray(dv.to_host(), dtype=np.uint64).reshape(-1)


def _round_trip(b, C, n, rounds, first_idx=0, num_clients=None, want_path="cohort-chain", prefer=None):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheClient, FlasheCohort
    cm.N_JOBS = 16
    num_clients = C if num_clients is None else num_clients
    sizes = _model_sizes(n)
    clients = []
    for c in range(C):
        cl = FlasheClient(_args(b))
        cl.create_cipher(first_idx + c, num_clients, KEY)
        clients.append(cl)
    co = FlasheCohort(_args(b), first_idx=first_idx, n_local=C, num_clients=num_clients, prp_seed=KEY, compact=True)
    co.prefer = prefer
    eng = co.cipher.engine
    for it in range(rounds):
        models = _host_models(C, sizes, 300 + it)
        for cl in clients:
            cl.set_iter_index(it)
        co.set_iter_index(it)
        np.random.seed(11 + it)
        np.random.random(5)
        state = np.random.get_state()
        want, want_state = _sequential(clients, models, True, state)
        want_sum = clients[0].cipher.aggregate(want)
        _poison(eng, [4 * n] * (C + 1))
        np.random.set_state(state)
        up = co.quantize_encrypt([_W(dict(m)) for m in models], normalize=True)
        assert up.path == want_path
        assert _same_state(np.random.get_state(), want_state), "the NumPy stream must be left where the sequential steps leave it"
        assert co.lead._cohort_mask is None
        for v in up.ciphertexts + [up.partial_sum]:
            assert v.compact and v.elem_bytes == 4 and len(v) == n
        for c in range(C):
            assert np.array_equal(_values_of(up.ciphertexts[c]), _values_of(want[c])), (it, c)
        assert np.array_equal(_values_of(up.partial_sum), _values_of(want_sum)), it
        agg = co.cipher.aggregate(up.ciphertexts, device=True)
        assert np.array_equal(_values_of(agg), _values_of(up.partial_sum))
        assert co.shape_dict == clients[0].shape_dict
        assert [float(a).hex() for a in co.quantizer.alpha_list] == [float(a).hex() for a in clients[0].quantizer.alpha_list]
        if num_clients != C:
            with pytest.raises(ValueError):
                co.decrypt_unquantize()
            return
        clients[0].set_idx_list(list(range(C)))
        ref = clients[0].decrypt_unquantize(_W({sorted(models[0])[0]: want_sum}), unnormalize=True)
        got = co.decrypt_unquantize(unnormalize=True)
        assert got.walking_order == ref.walking_order
        for k in ref.walking_order:
            assert np.asarray(got._weights[k]).shape == np.asarray(ref._weights[k]).shape
            assert np.asarray(got._weights[k], dtype=np.float64).tobytes() == np.asarray(ref._weights[k], dtype=np.float64).tobytes(), (it, k)
        qa, qb = co.quantizer, clients[0].quantizer
        assert [float(x).hex() for x in qa.past_layer_mean_list] == [float(x).hex() for x in qb.past_layer_mean_list]
        assert [float(x).hex() for x in qa.past_layer_std_list] == [float(x).hex() for x in qb.past_layer_std_list]
        for cl in clients[1:]:
            cl.quantizer.past_layer_mean_list = list(qb.past_layer_mean_list)
            cl.quantizer.past_layer_std_list = list(qb.past_layer_std_list)


def _admission(b):
    from flashe_amd.block import compact_cohort_admission_length
    return compact_cohort_admission_length(_cu_count(), b, 16)


@pytest.mark.parametrize("b", [20, 23])
def test_compact_cohort_is_the_sequential_clients_for_three_rounds(b):
    _round_trip(b, 3, _admission(b) + 12345, rounds=3)


def test_one_element_below_the_admission_length_takes_the_staged_chain():
    n = _admission(20)
    _round_trip(20, 3, n, rounds=1)
    _round_trip(20, 3, n - 1, rounds=1, want_path="staged-chain")


def test_a_cohort_inside_a_larger_federation_writes_a_partial_aggregate():
    _round_trip(20, 3, _admission(20) + 77, rounds=1, first_idx=3, num_clients=9)


@pytest.mark.parametrize("prefer", ["staged-chain", "per-client"])
def test_the_preferred_fallbacks_give_the_same_values(prefer):
    _round_trip(23, 3, _admission(23) + 5, rounds=1, want_path=prefer, prefer=prefer)


def test_compact_needs_a_compact_width():
    from flashe_amd.block import FlasheCohort
    with pytest.raises(ValueError, match="int_bits"):
        FlasheCohort(_args(128), first_idx=0, n_local=2, num_clients=2, prp_seed=KEY, compact=True)
    with pytest.raises(ValueError, match="int_bits"):
        FlasheCohort(_args(33), first_idx=0, n_local=2, num_clients=2, prp_seed=KEY, compact=True)
