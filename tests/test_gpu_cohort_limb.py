"""GPU: a cohort's chained launch from the floats at int_bits 33 .. 64 in the one-limb layout (flashe_quantize_encrypt_cohort_u64_dev,
prf_limb_cohort_kernel<2 | 3>; FlasheCohort(one_limb=True)).  ABI level on two CUs, where the launch admits 16-25 thousand values: every
ciphertext against the fused client step of that client in the same layout on the same engine with the same draws, the sum against the
mod-2^b sum of them in NumPy uint64, whole arrays, outputs poisoned with 0xA5 beforehand.  Class level at the chip's own admission
length against sequential FlasheClients (the path tests/golden/clientstep.json pins), everything compared as bytes or values and
`up.path` asserted everywhere."""
import numpy as np
import pytest

from test_gpu_cohort import KEY, _W, _args, _host_models, _poison, _same_state, _sequential

pytestmark = pytest.mark.gpu

# int_bits, element_bits: both M (3 up to 42, 2 from 43), the switch at 42 | 43, slots that straddle the 64-bit halves (40, 42, 48), the
# full-width mask (64)
WIDTHS = [(33, 29), (40, 32), (42, 38), (43, 39), (48, 40), (63, 59), (64, 60)]
CHUNKINGS = [(16, 2), (7, 10), (1, 1)]                                   # n_jobs, clients
POISON = np.uint64(0xA5A5A5A5A5A5A5A5)
HEAD = [1, 7, 0, 10007, 256 * 37 + 91]


@pytest.fixture(scope="module")
def E():
    from flashe_amd import engine
    return engine


def _length(b, J, cus=2, extra=0):
    """A length at or past the launch's admission on `cus` CUs with both kinds of chunks present where J > 1 (d + 1 and d elements).
    m = 3: neither is a multiple of m, so every chunk ends in a partial block, the tiles around the chunk ends walk and the last tile is
    partial.  m = 2: one of d and d + 1 is even whatever n is, so the chunks of one kind end in a partial block and those of the other in
    whole blocks that begin at odd elements; the last chunk is of the odd kind (d odd; J = 1: n odd)."""
    from flashe_amd.block import compact_cohort_admission_length
    m, n = 128 // b, compact_cohort_admission_length(cus, b, J) + extra
    n = max(n, sum(HEAD) + 1031 + extra)                  # (m = 2 admits 16,384 values on two CUs: room for the layer sizes below)
    if m == 2:
        while (J > 1 and n % J == 0) or (n // J) % 2 == 0:
            n += 1
        return n
    while (J > 1 and n % J == 0) or (n // J) % m == 0 or (n // J + 1) % m == 0:
        n += 1
    return n


def _sizes(n):
    """Rows that begin inside a block and inside a half tile, an empty row.  (A vector at the m = 2 admission length itself is shorter than
    these five: it keeps the first four.)"""
    head = HEAD if n > sum(HEAD) else HEAD[:4]
    return head + [n - sum(head)]


def _values(dtype, alpha, size, seed):
    """Values inside the clip range with the edges strewn in: beyond +-alpha, exactly +-alpha, 0, the float below alpha."""
    g = np.random.Generator(np.random.PCG64(seed))
    x = (g.standard_normal(size) * alpha / 2).astype(dtype)
    for k, v in enumerate((alpha, -alpha, 0.0, 3 * alpha, -3 * alpha, np.nextafter(dtype(alpha), dtype(0)))):
        x[k::89] = v
    return x


def _cohort_case(E, eng, b, bits, J, C, n, it=3, first_idx=5, alias=False):
    """The shared rows, every client's sources and draws, and the per-client reference: quantize_encrypt_model_dev on the same engine with
    the same draws."""
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


def _outputs(E, eng, C, n, offset):
    """C + 1 poisoned n-element uint64 vectors; offset 8: each one a view 8 bytes into a larger buffer (8 bytes past a 16-byte boundary)."""
    bufs = [eng.alloc(8 * n + 16) for _ in range(C + 1)]
    for d in bufs:
        eng.memset_dev(d, 0xA5, 8 * n + 16)
    views = [E.DeviceBufferView(d, offset, 8 * n) if offset else d for d in bufs]
    return bufs, views


def _run(E, eng, b, bits, J, C, n, alias=False, it=3, first_idx=5, offset=0):
    rows, srcs, dts, du, want, keep = _cohort_case(E, eng, b, bits, J, C, n, it, first_idx, alias)
    bufs, views = _outputs(E, eng, C, n, offset)
    ok = eng.quantize_encrypt_cohort_u64_dev(it, first_idx, n, J, rows, srcs, dts, bits, du, views[:C], views[C])
    whole = [d.download(np.uint64, n + 2).copy() for d in bufs]
    at = offset // 8
    for w in whole:                                         # what lies around the vectors stays poisoned
        assert (w[:at] == POISON).all() and (w[at + n:] == POISON).all()
    got = [w[at:at + n] for w in whole]
    del keep
    return ok, got[:C], got[C], want


def _check(got, gsum, want, b, *what):
    total = np.zeros(len(gsum), dtype=np.uint64)
    for c, (g, w) in enumerate(zip(got, want)):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, "client", c, bad[:6], g[bad[:6]], w[bad[:6]], bad.size)
        total += w
    if b < 64:
        total &= np.uint64((1 << b) - 1)
    bad = np.flatnonzero(gsum != total)
    assert bad.size == 0, (what, "sum", bad[:6], gsum[bad[:6]], total[bad[:6]], bad.size)


def _untouched(got, gsum):
    return all((g == POISON).all() for g in got + [gsum])


# ------------------------------------------------------------------------------------------------ ABI level, two CUs
@pytest.mark.parametrize("J,C", CHUNKINGS)
@pytest.mark.parametrize("b,bits", WIDTHS)
def test_the_one_limb_launch_is_every_clients_fused_step(E, b, bits, J, C):
    eng = E.Engine(KEY, b, device=0)
    eng.set_cu_limit(2)
    n = _length(b, J, extra=777)
    ok, got, gsum, want = _run(E, eng, b, bits, J, C, n)
    assert ok, "the chained one-limb cohort launch declined the shape"
    _check(got, gsum, want, b, b, J, C, n)


@pytest.mark.parametrize("J", [16, 7, 1])
@pytest.mark.parametrize("C", [1, 10])
@pytest.mark.parametrize("b,bits", [(40, 32), (64, 60)])
def test_two_and_eleven_streams_under_every_chunking(E, b, bits, C, J):
    eng = E.Engine(KEY, b, device=0)
    eng.set_cu_limit(2)
    n = _length(b, J)
    ok, got, gsum, want = _run(E, eng, b, bits, J, C, n)
    assert ok
    _check(got, gsum, want, b, J, C, n)


@pytest.mark.parametrize("C", [128, 129])
def test_the_link_table_boundary(E, C):
    """kMaxLinks clients chain; one more is FLASHE_ENOTSUP with the outputs untouched.  Every client reads client 0's model."""
    eng = E.Engine(KEY, 40, device=0)
    eng.set_cu_limit(2)
    n = _length(40, 16)
    ok, got, gsum, want = _run(E, eng, 40, 32, 16, C, n, alias=True)
    if C == 128:
        assert ok
        _check(got, gsum, want, 40, C)
    else:
        assert ok is False
        assert _untouched(got, gsum)


@pytest.mark.parametrize("b,bits", [(40, 32), (64, 60)])
def test_outputs_eight_bytes_past_a_sixteen_byte_boundary(E, b, bits):
    eng = E.Engine(KEY, b, device=0)
    eng.set_cu_limit(2)
    n = _length(b, 16, extra=131)
    ok, got, gsum, want = _run(E, eng, b, bits, 16, 3, n, offset=8)
    assert ok
    _check(got, gsum, want, b, "offset 8")


def test_the_last_prefix_is_refused(E):
    """first_idx + C - 1 = 2^32 - 1: the double mask's idx + 1 does not fit the prefix field."""
    eng = E.Engine(KEY, 40, device=0)
    eng.set_cu_limit(2)
    n = _length(40, 16)
    rows, srcs, dts, du, _want, keep = _cohort_case(E, eng, 40, 32, 16, 2, n, first_idx=2 ** 32 - 3)
    bufs, _views = _outputs(E, eng, 2, n, 0)
    with pytest.raises(E.FlasheError) as ei:
        eng.quantize_encrypt_cohort_u64_dev(3, 2 ** 32 - 2, n, 16, rows, srcs, dts, 32, du, bufs[:2], bufs[2])
    assert ei.value.code == -22
    assert _untouched([d.download(np.uint64, n) for d in bufs[:2]], bufs[2].download(np.uint64, n))
    del keep
    ok, got, gsum, want = _run(E, eng, 40, 32, 16, 2, n, first_idx=2 ** 32 - 3)
    assert ok
    _check(got, gsum, want, 40, "top")


@pytest.mark.parametrize("b,bits", [(40, 32), (64, 60)])
def test_one_value_below_admission_is_declined_untouched(E, b, bits):
    from flashe_amd.block import compact_cohort_admission_length
    eng = E.Engine(KEY, b, device=0)
    eng.set_cu_limit(2)
    n = compact_cohort_admission_length(2, b, 16)
    ok, got, gsum, want = _run(E, eng, b, bits, 16, 3, n)
    assert ok
    _check(got, gsum, want, b, "at admission")
    ok, got, gsum, _want = _run(E, eng, b, bits, 16, 3, n - 1)
    assert ok is False
    assert _untouched(got, gsum)


@pytest.mark.parametrize("b,bits", [(32, 24), (65, 60)])
def test_a_ctx_of_another_width_declines_untouched(E, b, bits):
    from flashe_amd import _lib
    eng = E.Engine(KEY, b, device=0)
    eng.set_cu_limit(2)
    n = _length(33, 16, extra=5000)
    x, u = eng.upload(np.zeros(n, np.float32)), eng.upload(np.zeros(n))
    # (two-limb ctx: 16 bytes per element, 16-byte aligned, so that only the width stands against the launch)
    ct, dsum = eng.alloc(16 * n), eng.alloc(16 * n)
    for d in (ct, dsum):
        eng.memset_dev(d, 0xA5, 16 * n)
    assert eng.quantize_encrypt_cohort_u64_dev(0, 0, n, 16, [(0, None, 1.0, 0.0, _lib.TENSOR_F32, 0)], [[x.ptr]], [[_lib.TENSOR_F32]], bits, u, [ct], dsum) is False
    assert _untouched([ct.download(np.uint64, 2 * n)], dsum.download(np.uint64, 2 * n))


def test_staged_sources_float16_bfloat16_shift(E):
    """Sources that are not read in place take the one stage pass: float16 and bfloat16 storage, float32 under a float64 row, SHIFT.
    The reference is quantize_encrypt_tensors_dev of each client (which stages the same way)."""
    from flashe_amd import _lib
    b, bits, J, C, it = 40, 32, 16, 3, 9
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
    bufs, _views = _outputs(E, eng, C, n, 0)
    assert eng.quantize_encrypt_cohort_u64_dev(it, 1, n, J, rows, srcs, dts, bits, du, bufs[:C], bufs[C])
    _check([d.download(np.uint64, n).copy() for d in bufs[:C]], bufs[C].download(np.uint64, n).copy(), want, b, "staged")


# ------------------------------------------------------------------------------------------------ class level, the chip's admission length
def _cu_count():
    from flashe_amd import Engine
    return Engine(KEY, 40).cu_count


def _model_sizes(n):
    head = [1, 7, 0, 10007, 256 * 37 + 91]
    rest = n - sum(head)
    cuts = [rest // 7, rest // 3 + 5]
    return head + cuts + [rest - sum(cuts)]


def _values_of(dv):
    return np.asarray(dv.to_host(), dtype=np.uint64).reshape(-1)


def _round_trip(b, eb, C, n, rounds, first_idx=0, num_clients=None, want_path="cohort-chain", prefer=None):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheClient, FlasheCohort
    cm.N_JOBS = 16
    num_clients = C if num_clients is None else num_clients
    sizes = _model_sizes(n)
    clients = []
    for c in range(C):
        cl = FlasheClient(_args(b, eb))
        cl.create_cipher(first_idx + c, num_clients, KEY)
        clients.append(cl)
    co = FlasheCohort(_args(b, eb), first_idx=first_idx, n_local=C, num_clients=num_clients, prp_seed=KEY, one_limb=True)
    assert co.one_limb
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
        _poison(eng, [8 * n] * (C + 1))
        np.random.set_state(state)
        up = co.quantize_encrypt([_W(dict(m)) for m in models], normalize=True)
        assert up.path == want_path
        assert _same_state(np.random.get_state(), want_state), "the NumPy stream must be left where the sequential steps leave it"
        assert co.lead._cohort_mask is None
        for v in up.ciphertexts + [up.partial_sum]:
            assert not getattr(v, "compact", False) and v.elem_bytes == 8 and len(v) == n
        for c in range(C):
            assert np.array_equal(_values_of(up.ciphertexts[c]), _values_of(want[c])), (it, c)
        assert np.array_equal(_values_of(up.partial_sum), _values_of(want_sum)), it
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


def test_one_limb_cohort_is_the_sequential_clients_for_three_rounds():
    """int_bits 36: element_bits 32 and three clients, the job that quantises finer than the compact chain carries."""
    _round_trip(36, 32, 3, _admission(36) + 12345, rounds=3)


def test_one_limb_cohort_at_int_bits_64():
    _round_trip(64, 48, 3, _admission(64) + 12345, rounds=1)


def test_one_value_below_the_admission_length_takes_the_staged_chain():
    n = _admission(36)
    _round_trip(36, 32, 3, n, rounds=1)
    _round_trip(36, 32, 3, n - 1, rounds=1, want_path="staged-chain")


def test_a_cohort_inside_a_larger_federation_writes_a_partial_aggregate():
    _round_trip(36, 32, 3, _admission(36) + 77, rounds=1, first_idx=3, num_clients=9)


@pytest.mark.parametrize("prefer", ["staged-chain", "per-client"])
def test_the_preferred_fallbacks_give_the_same_values(prefer):
    _round_trip(36, 32, 3, _admission(36) + 5, rounds=1, want_path=prefer, prefer=prefer)


def test_one_limb_needs_a_one_limb_width():
    from flashe_amd.block import FlasheCohort
    for b in (32, 65, 128):
        with pytest.raises(ValueError, match="int_bits"):
            FlasheCohort(_args(b), first_idx=0, n_local=2, num_clients=2, prp_seed=KEY, one_limb=True)
