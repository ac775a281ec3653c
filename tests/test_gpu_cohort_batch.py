"""GPU: a cohort's chained launch from the floats for a BATCHED job at int_bits > 64 (flashe_quantize_batch_encrypt_cohort_dev,
prf_chain_cohort_batch_kernel<1024, 5 / 6 / 7>) and the batched back end over caller-held masks
(flashe_combine_unbatch_unquantize_model_dev).  ABI level on two CUs, where the launch admits 16,129 batched elements: every ciphertext
against flashe_quantize_batch_tensors_dev + flashe_encrypt_dev of that client on the same engine, the sum against the mod-2^b sum of
them, the mask against the library's decrypt.  Class level at the chip's own admission length against sequential FlasheClients.
Everything is compared as bytes and the outputs are poisoned before every call."""
import numpy as np
import pytest

from test_gpu_cohort import KEY, _W, _args, _poison, _same_state, _sequential
from test_gpu_cohort_compact import _values

pytestmark = pytest.mark.gpu

SHAPES = [(120, 10, 6), (128, 3, 7), (120, 20, 5), (128, 10, 6)]       # int_bits, num_clients -> bs at element_bits 16
J = 16


@pytest.fixture(scope="module")
def E():
    from flashe_amd import engine
    return engine


def _field_bits(num_clients, element_bits=16):
    return element_bits + int(np.ceil(np.log2(num_clients)))


def _elems_to_sizes(bs, n_elems):
    """Layers whose batched elements are n_elems in all: one value (an element with bs - 1 pads), an empty layer, sizes = 0, 1 and
    bs - 1 mod bs; layers 2 and 3 start inside a pair (elements 1 and 101), layer 4 on element 128, layer 5 on element 768 = 3 x 256."""
    elems = [1, 0, 100, 27, 640, 5001]
    sizes = [1, 0, 100 * bs, 26 * bs + 1, 639 * bs + bs - 1, 5000 * bs + 2]
    rest = n_elems - sum(elems)
    assert rest > 0
    sizes.append(rest * bs - (bs - 2))
    assert sum(-(-s // bs) for s in sizes) == n_elems
    return sizes


def _to_ints(a):
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 2)
    return a[:, 0].astype(object) + (a[:, 1].astype(object) << 64)


def _from_ints(v):
    out = np.empty((len(v), 2), dtype=np.uint64)
    out[:, 0] = (v & ((1 << 64) - 1)).astype(np.uint64)
    out[:, 1] = (v >> 64).astype(np.uint64)
    return out


class _Case:
    """The shared rows, every client's sources and draws, and the per-client reference (plaintext and ciphertext) of one cohort."""

    def __init__(self, E, eng, b, num_clients, C, n_elems, first_idx=5, it=3, alias=False, element_bits=16, field_bits=None, sizes=None):
        from flashe_amd import _lib
        self.b, self.C, self.it, self.first_idx, self.n_elems, self.bits = b, C, it, first_idx, n_elems, element_bits
        self.fb = field_bits or _field_bits(num_clients, element_bits)
        self.bs = b // self.fb
        self.sizes = sizes or _elems_to_sizes(self.bs, n_elems)
        self.n = sum(self.sizes)
        alphas = [0.37, 2.5, 1.0, 8.17121, 3e-3, 0.05, 0.6]
        starts = np.concatenate([[0], np.cumsum(self.sizes)[:-1]]).tolist()
        f64 = [bool(li % 2) for li in range(len(self.sizes))]
        self.rows = [(starts[li], None, alphas[li], 0.0, _lib.TENSOR_F64 if f64[li] else _lib.TENSOR_F32, 0) for li in range(len(self.sizes))]
        u = np.random.Generator(np.random.PCG64(b * 1000 + C)).random(C * self.n)
        u[::5] = 0.0
        u[1::5] = 1.0 - 2.0 ** -53
        self.du = eng.upload(u)
        self.srcs, self.dts, self.keep, self.pts, self.want = [], [], [], [], []
        for c in range(C):
            if alias and c:
                self.srcs.append(self.srcs[0])
                self.dts.append(self.dts[0])
            else:
                xs = [_values(np.float64 if f64[li] else np.float32, alphas[li], size, 100 * c + li) for li, size in enumerate(self.sizes)]
                ds = [eng.upload(x) if x.size else eng.alloc(16) for x in xs]
                self.keep += ds
                self.srcs.append([d.ptr for d in ds])
                self.dts.append([r[4] for r in self.rows])
            table = [(starts[li], self.srcs[c][li], alphas[li], 0.0, self.rows[li][4], 0) for li in range(len(self.sizes))]
            pt, ref = eng.alloc_vec(n_elems), eng.alloc_vec(n_elems)
            eng.quantize_batch_tensors_dev(table, self.n, element_bits, self.fb, self.du.ptr + 8 * c * self.n, n_elems, pt)
            eng.encrypt_dev(it, first_idx + c, E.SCHEME_DOUBLE, n_elems, J, pt, 2, ref)
            self.pts.append(pt.download(np.uint64, 2 * n_elems).copy())
            self.want.append(ref.download(np.uint64, 2 * n_elems).copy())

    def run(self, eng, dmask=True, n_elems=None, first_idx=None):
        n_elems = self.n_elems if n_elems is None else n_elems
        outs = [eng.alloc_vec(self.n_elems) for _ in range(self.C + 2)]
        for d in outs:
            eng.memset_dev(d, 0xA5, 16 * self.n_elems)
        ok = eng.quantize_batch_encrypt_cohort_dev(self.it, self.first_idx if first_idx is None else first_idx, self.n, n_elems, J, self.rows, self.srcs,
                                                   self.dts, self.bits, self.fb, self.du, outs[:self.C], outs[self.C], outs[self.C + 1] if dmask else None)
        got = [d.download(np.uint64, 2 * self.n_elems).copy() for d in outs]
        return ok, got[:self.C], got[self.C], got[self.C + 1]

    def want_sum(self):
        total = sum(_to_ints(w) for w in self.want) & ((1 << self.b) - 1)
        return _from_ints(total).reshape(-1)


def _same(got, want, *what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad[:6] // 2, [hex(int(v)) for v in got[bad[:6]]], [hex(int(v)) for v in want[bad[:6]]], bad.size)


def _untouched(*arrays):
    return all((a == np.uint64(0xA5A5A5A5A5A5A5A5)).all() for a in arrays)


def _admission(cus=2):
    from flashe_amd.block import cohort_admission_length
    return cohort_admission_length(cus)


# ------------------------------------------------------------------------------------------------ ABI level, two CUs
@pytest.mark.parametrize("C", [1, 2, 10])
@pytest.mark.parametrize("b,num_clients,bs", SHAPES)
def test_the_batched_launch_is_every_clients_quantise_batch_encrypt(E, b, num_clients, bs, C):
    eng = E.Engine(KEY, b, device=0)
    eng.set_cu_limit(2)
    case = _Case(E, eng, b, num_clients, C, _admission() + 777)
    assert case.bs == bs
    ok, got, gsum, _mask = case.run(eng)
    assert ok, "the chained batched cohort launch declined the shape"
    for c in range(C):
        _same(got[c], case.want[c], b, bs, C, "client", c)
    _same(gsum, case.want_sum(), b, bs, C, "sum")


@pytest.mark.parametrize("b,num_clients,bs", SHAPES[:3])
def test_the_decrypt_mask(E, b, num_clients, bs):
    """(sum + mask) mod 2^b is the sum of the clients' batched plaintexts and the library's decrypt of the sum; without a mask the other
    outputs are the same."""
    C = 3
    eng = E.Engine(KEY, b, device=0)
    eng.set_cu_limit(2)
    case = _Case(E, eng, b, num_clients, C, _admission() + 777, first_idx=0)
    ok, got, gsum, mask = case.run(eng)
    assert ok
    opened = _from_ints((_to_ints(gsum) + _to_ints(mask)) & ((1 << b) - 1)).reshape(-1)
    plain = _from_ints(sum(_to_ints(p) for p in case.pts) & ((1 << b) - 1)).reshape(-1)
    _same(opened, plain, b, "sum + mask against the plaintexts")
    dsum, dec = eng.upload(gsum), eng.alloc_vec(case.n_elems)
    eng.decrypt_dev(case.it, [C], [0], case.n_elems, J, dsum, dec)
    _same(opened, dec.download(np.uint64, 2 * case.n_elems), b, "sum + mask against the decrypt")
    ok, got2, gsum2, mask2 = case.run(eng, dmask=False)
    assert ok and _untouched(mask2)
    for c in range(C):
        _same(got2[c], got[c], b, "client without a mask", c)
    _same(gsum2, gsum, b, "sum without a mask")


def test_staged_sources_bfloat16_with_shift(E):
    """Sources that are not read in place take the one stage pass: bfloat16 storage normalised with SHIFT, every client's own; the
    reference is quantize_batch_tensors_dev given the same table."""
    from flashe_amd import _lib
    b, num_clients, C, it, first_idx = 120, 10, 3, 9, 2
    eng = E.Engine(KEY, b, device=0)
    eng.set_cu_limit(2)
    fb = _field_bits(num_clients)
    bs = b // fb
    n_elems = _admission() + 300
    sizes = [4097, 3, 0, (n_elems - 683 - 1) * bs - 1]
    assert sum(-(-s // bs) for s in sizes) == n_elems
    n = sum(sizes)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    shifts, alpha = [0.0625, -0.25, 0.0, 0.125], 1.5
    rows = [(starts[li], None, alpha, shifts[li], _lib.TENSOR_F32, _lib.TENSOR_SHIFT) for li in range(len(sizes))]
    du = eng.upload(np.random.Generator(np.random.PCG64(5)).random(C * n))
    srcs, dts, keep, want = [], [], [], []
    for c in range(C):
        ds = []
        for li, size in enumerate(sizes):
            x = _values(np.float32, alpha, size, 50 * c + li)
            ds.append(eng.upload((np.ascontiguousarray(x).view(np.uint32) >> np.uint32(16)).astype(np.uint16)) if size else eng.alloc(16))
        keep += ds
        srcs.append([d.ptr for d in ds])
        dts.append([_lib.TENSOR_BF16] * len(sizes))
        table = [(starts[li], srcs[c][li], alpha, shifts[li], _lib.TENSOR_BF16, _lib.TENSOR_SHIFT) for li in range(len(sizes))]
        pt, ref = eng.alloc_vec(n_elems), eng.alloc_vec(n_elems)
        eng.quantize_batch_tensors_dev(table, n, 16, fb, du.ptr + 8 * c * n, n_elems, pt)
        eng.encrypt_dev(it, first_idx + c, E.SCHEME_DOUBLE, n_elems, J, pt, 2, ref)
        want.append(ref.download(np.uint64, 2 * n_elems).copy())
    outs = [eng.alloc_vec(n_elems) for _ in range(C + 1)]
    for d in outs:
        eng.memset_dev(d, 0xA5, 16 * n_elems)
    assert eng.quantize_batch_encrypt_cohort_dev(it, first_idx, n, n_elems, J, rows, srcs, dts, 16, fb, du, outs[:C], outs[C])
    for c in range(C):
        _same(outs[c].download(np.uint64, 2 * n_elems), want[c], "bfloat16 + SHIFT", c)
    total = _from_ints(sum(_to_ints(w) for w in want) & ((1 << b) - 1)).reshape(-1)
    _same(outs[C].download(np.uint64, 2 * n_elems), total, "bfloat16 + SHIFT sum")


# ------------------------------------------------------------------------------------------------ refusals
def test_one_element_below_admission_is_declined_untouched(E):
    eng = E.Engine(KEY, 120, device=0)
    eng.set_cu_limit(2)
    at = _Case(E, eng, 120, 10, 2, _admission(), sizes=[6 * _admission()])
    ok, got, gsum, mask = at.run(eng)
    assert ok
    _same(got[1], at.want[1], "at the admission length")
    _same(gsum, at.want_sum(), "at the admission length: sum")
    below = _Case(E, eng, 120, 10, 2, _admission() - 1, sizes=[6 * (_admission() - 1)])
    ok, got, gsum, mask = below.run(eng)
    assert ok is False and _untouched(*got, gsum, mask)


@pytest.mark.parametrize("C", [128, 129])
def test_the_link_table_boundary(E, C):
    """kMaxLinks clients chain; one more is FLASHE_ENOTSUP with the outputs untouched.  Every client reads client 0's model."""
    eng = E.Engine(KEY, 120, device=0)
    eng.set_cu_limit(2)
    case = _Case(E, eng, 120, 20, C, _admission() + 5, first_idx=0, alias=True, sizes=[5 * (_admission() + 5) - 2])
    ok, got, gsum, mask = case.run(eng)
    if C == 128:
        assert ok
        for c in (0, 1, 64, 127):
            _same(got[c], case.want[c], "client", c)
        _same(gsum, case.want_sum(), "sum of 128")
    else:
        assert ok is False and _untouched(*got, gsum, mask)


def test_shapes_outside_the_launch_are_declined_untouched(E):
    from flashe_amd import _lib
    n_elems = _admission() + 5
    # int_bits 64 (one limb; 6 values of 8 + 2 bits per element)
    eng = E.Engine(KEY, 64, device=0)
    eng.set_cu_limit(2)
    n = 6 * n_elems
    x, u = eng.upload(np.zeros(n, np.float32)), eng.upload(np.zeros(2 * n))
    outs = [eng.alloc(16 * n_elems) for _ in range(4)]
    for d in outs:
        eng.memset_dev(d, 0xA5, 16 * n_elems)
    rows = [(0, None, 1.0, 0.0, _lib.TENSOR_F32, 0)]
    assert eng.quantize_batch_encrypt_cohort_dev(0, 0, n, n_elems, J, rows, [[x.ptr]] * 2, [[_lib.TENSOR_F32]] * 2, 8, 10, u, outs[:2], outs[2], outs[3]) is False
    assert _untouched(*[d.download(np.uint64, 2 * n_elems) for d in outs])
    # element_bits 8 at int_bits 120 and ten clients: bs 10
    eng = E.Engine(KEY, 120, device=0)
    eng.set_cu_limit(2)
    case = _Case(E, eng, 120, 10, 2, n_elems, element_bits=8, sizes=[10 * n_elems - 3])
    assert case.bs == 10
    ok, got, gsum, mask = case.run(eng)
    assert ok is False and _untouched(*got, gsum, mask)


def test_bad_arguments_are_einval(E):
    eng = E.Engine(KEY, 120, device=0)
    eng.set_cu_limit(2)
    case = _Case(E, eng, 120, 10, 2, _admission() + 5, sizes=[6 * (_admission() + 5)])
    for kw in ({"first_idx": 2 ** 32 - 2}, {"n_elems": case.n_elems + 1}, {"n_elems": case.n_elems - 1}):
        with pytest.raises(E.FlasheError) as ei:
            case.run(eng, **kw)
        assert ei.value.code == -22, kw
    ok, got, gsum, _mask = case.run(eng, first_idx=2 ** 32 - 3)
    assert ok
    ref = eng.alloc_vec(case.n_elems)
    eng.encrypt_dev(case.it, 2 ** 32 - 2, E.SCHEME_DOUBLE, case.n_elems, J, eng.upload(case.pts[1]), 2, ref)
    _same(got[1], ref.download(np.uint64, 2 * case.n_elems), "the last admissible prefix")


# ------------------------------------------------------------------------------------------------ the batched back end
@pytest.mark.parametrize("with_minus", [True, False])
@pytest.mark.parametrize("b,num_clients,bs", [(120, 10, 6), (128, 3, 7)])
def test_combine_unbatch_unquantize_is_decrypt_then_unbatch_unquantize(E, b, num_clients, bs, with_minus):
    eng = E.Engine(KEY, b, device=0)
    fb = _field_bits(num_clients)
    sizes = [1, 0, 100 * bs, 26 * bs + 1, 639 * bs + bs - 1, 3000 * bs + 2]
    layers = [(s, None, 0.3 + 0.1 * li, False) for li, s in enumerate(sizes)]
    n_elems, n, it = sum(-(-s // bs) for s in sizes), sum(sizes), 6
    g = np.random.Generator(np.random.PCG64(b + with_minus))
    raw = g.integers(0, 2 ** 64, (n_elems, 2), dtype=np.uint64)
    raw[:, 1] &= np.uint64((1 << (b - 64)) - 1)
    din = eng.upload(raw)
    add_idx, minus_idx = [num_clients], ([0] if with_minus else [])
    dec, want = eng.alloc_vec(n_elems), eng.alloc(8 * n)
    eng.decrypt_dev(it, add_idx, minus_idx, n_elems, J, din, dec)
    eng.unbatch_unquantize_model_dev(layers, 16, fb, num_clients, dec, n_elems, want)
    add, minus = eng.alloc_vec(n_elems), (eng.alloc_vec(n_elems) if with_minus else None)
    eng.mask_dev(it, add_idx, n_elems, J, add)
    if with_minus:
        eng.mask_dev(it, minus_idx, n_elems, J, minus)
    got = eng.alloc(8 * n)
    eng.memset_dev(got, 0xA5, 8 * n)
    eng.combine_unbatch_unquantize_model_dev(layers, 16, fb, num_clients, din, add, minus, n_elems, got)
    assert got.download(np.float64, n).tobytes() == want.download(np.float64, n).tobytes()
    # no masks at all: the plain unbatch + unquantise
    eng.unbatch_unquantize_model_dev(layers, 16, fb, num_clients, din, n_elems, want)
    eng.combine_unbatch_unquantize_model_dev(layers, 16, fb, num_clients, din, None, None, n_elems, got)
    assert got.download(np.float64, n).tobytes() == want.download(np.float64, n).tobytes()
    with pytest.raises(E.FlasheError) as ei:
        eng.combine_unbatch_unquantize_model_dev(layers, 16, fb, num_clients, din, add, minus, n_elems + 1, got)
    assert ei.value.code == -22


# ------------------------------------------------------------------------------------------------ class level, the whole chip
def _cu_count():
    from flashe_amd import Engine
    return Engine(KEY, 128).cu_count


def _models(C, sizes, seed):
    """One model per client: client 0's values (float32 and float64 layers alternating, some beyond the clip range) shifted per client."""
    g = np.random.Generator(np.random.PCG64(seed))
    base = [(g.standard_normal(s, dtype=np.float32) * np.float32(0.05)).astype(np.float64 if i % 2 else np.float32) for i, s in enumerate(sizes)]
    return [{f"l{i:02d}": (x + x.dtype.type(0.01 * c)).reshape((s,) if i % 2 else (1, s)) for i, (x, s) in enumerate(zip(base, sizes))} for c in range(C)]


def _class_round_trip(C, rounds, prefer=None):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheClient, FlasheCohort, cohort_admission_length
    cm.N_JOBS = 16
    bs = 120 // _field_bits(C)
    n_elems = cohort_admission_length(_cu_count()) + 300
    head = [1, 10007, 256 * 37 + 91, 0]
    sizes = head + [bs * n_elems - sum(head)]
    clients = []
    for c in range(C):
        cl = FlasheClient(_args(120, 16, True))
        cl.create_cipher(c, C, KEY)
        clients.append(cl)
    co = FlasheCohort(_args(120, 16, True), first_idx=0, n_local=C, num_clients=C, prp_seed=KEY)
    co.prefer = prefer
    eng = co.cipher.engine
    out = []
    for it in range(rounds):
        normalize = it == 1
        models = _models(C, sizes, 100 + it)
        for cl in clients:
            cl.set_iter_index(it)
        co.set_iter_index(it)
        np.random.seed(7 + it)
        np.random.random(3)                                   # an odd position in the stream
        state = np.random.get_state()
        want, want_state = _sequential(clients, models, normalize, state)
        want_sum = clients[0].cipher.aggregate(want)
        n_got = len(want_sum)
        assert n_got >= n_elems
        _poison(eng, [16 * n_got] * (C + 2))
        np.random.set_state(state)
        up = co.quantize_encrypt([_W(dict(m)) for m in models], normalize=normalize)
        assert up.path == (prefer or "cohort-chain")
        assert _same_state(np.random.get_state(), want_state), "the NumPy stream must be left where the sequential steps leave it"
        for c in range(C):
            assert up.ciphertexts[c].to_host().tobytes() == want[c].to_host().tobytes(), (it, c)
        assert up.partial_sum.to_host().tobytes() == want_sum.to_host().tobytes(), it
        assert co.shape_dict == clients[0].shape_dict
        assert [float(a).hex() for a in co.quantizer.alpha_list] == [float(a).hex() for a in clients[0].quantizer.alpha_list]
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
        for cl in clients[1:]:                                # every client of the federation decrypts the same model: one state
            cl.quantizer.past_layer_mean_list = list(qb.past_layer_mean_list)
            cl.quantizer.past_layer_std_list = list(qb.past_layer_std_list)
        out.append((co.lead._cohort_mask is not None))
    return out


@pytest.mark.parametrize("C", [2, 3])
def test_the_batched_cohort_is_the_sequential_clients_for_two_rounds(C):
    """int_bits 120, batched (C = 2: 7 values per element, C = 3: 6), just past the chip's admission length; the second round
    normalises.  The decrypt of the cohort's own sum takes the mask the launch wrote."""
    assert _class_round_trip(C, rounds=2) == [True, True]


def test_prefer_staged_chain_gives_the_same_bytes():
    assert _class_round_trip(2, rounds=1, prefer="staged-chain") == [False]
