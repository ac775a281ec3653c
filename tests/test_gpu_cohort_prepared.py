"""GPU, ABI level: a precompute job's cohort.  The mask chain (C + 1 streams into caller-owned vectors: flashe_prf_jobs_dev with linked
input-less jobs in the limb layout, flashe_cohort_masks_u32_dev in the compact one) against single streams differenced on the host, and
the online launch (flashe_quantize_combine_cohort_dev / _u32_dev / flashe_quantize_batch_combine_cohort_dev: C float models + C masks ->
C ciphertexts + their sum, no AES) against the non-precompute fused client step of every client on the same engine with the same draws,
against host integer arithmetic on hand-made masks at the carry and wrap edges, over more clients than an argument block carries, with
a null sum, on an empty model, and its refusals.  Everything is compared as integer arrays; outputs are poisoned with 0xA5 first."""
import numpy as np
import pytest

from test_gpu_cohort import KEY
from test_gpu_cohort_batch import _Case, _from_ints, _to_ints
from test_gpu_cohort_compact import _values

pytestmark = pytest.mark.gpu

ALPHAS = [0.37, 2.5, 1.0, 8.17121, 3e-3, 0.05, 0.6]
# the issue's layers, and the same moved by one value so that no layer but the first starts on a multiple of 4 (1 + 7 = 8 does)
HEADS = [[1, 7, 0, 10007, 256 * 37 + 91], [1, 6, 0, 10007, 256 * 37 + 91]]
N = 30001                                                             # not a multiple of 4: the last run of four is partial


@pytest.fixture(scope="module")
def E():
    from flashe_amd import engine
    return engine


def _sizes(head, n=N):
    return head + [n - sum(head)]


def _elem_bytes(eng, compact):
    return 4 if compact else 8 * eng.limbs


def _alloc(eng, n, compact, fill=0xA5):
    nbytes = max(n * _elem_bytes(eng, compact), 16)
    d = eng.alloc(nbytes)
    eng.memset_dev(d, fill, nbytes)
    return d


def _get(eng, d, n, compact):
    """a vector as uint64 words: [n] values (compact, one limb) or [2 n] limbs"""
    if compact:
        return d.download(np.uint32, n).astype(np.uint64)
    return d.download(np.uint64, n * eng.limbs).copy()


def _ints(a, L):
    return _to_ints(a) if L == 2 else np.asarray(a, dtype=np.uint64).astype(object)


def _words(v, L):
    return _from_ints(v).reshape(-1) if L == 2 else np.array([int(x) for x in v], dtype=np.uint64)


def _same(got, want, *what):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    assert bad.size == 0, (what, bad[:6], [hex(int(v)) for v in got[bad[:6]]], [hex(int(v)) for v in want[bad[:6]]], bad.size)


def _host_sum(cts, b, L):
    return _words(sum(_ints(c, L) for c in cts) & ((1 << b) - 1), L)


# ------------------------------------------------------------------------------------------------ 1. the mask chain
def _chain_length(b, J, base):
    """The first length from `base` on whose n_jobs chunks end in partial AES blocks of m = 128 // b elements: chunks of d and of d + 1
    elements both present where J > 1; both kinds partial, or at m = 2 -- where one of d and d + 1 is even -- one of them."""
    m = max(128 // b, 1)
    for n in range(base, base + 64 * J * m):
        d, r = divmod(n, J)
        kinds = [d, d + 1] if r else [d]
        if m == 1 or ((J == 1 or r) and (all if m > 2 else any)(k % m for k in kinds)):
            return n
    raise AssertionError((b, J, base))


CHAIN = [(128, False), (120, False), (64, False), (33, False), (20, False), (16, True), (20, True), (23, True), (24, True), (32, True), (27, True)]


@pytest.mark.parametrize("J", [1, 7, 16])
@pytest.mark.parametrize("b,compact", CHAIN)
def test_the_mask_chain_is_the_difference_of_single_streams(E, b, compact, J):
    """C = 1, 2 and 10 from first_idx 0 and 5 against mask_dev's single streams differenced on the host.  int_bits 27 has no compiled
    width in the compact chain, which serves it through its run-time width.  C = 10 at a length past the paired kernel's admission on two
    CUs (the kernel a model-sized chain runs), the others a few thousand elements."""
    from flashe_amd.block import compact_cohort_admission_length
    it = 7
    eng = E.Engine(KEY, b, device=0)
    eng.set_cu_limit(2)
    L = eng.limbs
    assert not compact or eng.compact_supported()
    long_n = _chain_length(b, J, (compact_cohort_admission_length(2, b, J) if b <= 32 else 16129) + 333)
    short_n = _chain_length(b, J, 3001)
    M = (1 << b) - 1
    for n, combos in ((short_n, [(1, 0), (1, 5), (2, 0), (2, 5), (10, 5)]), (long_n, [(10, 0)])):
        streams = []
        for idx in range(16):
            d = eng.alloc_vec(n)
            eng.mask_dev(it, [idx], n, J, d)
            streams.append(_ints(d.download(np.uint64, n * L), L))
        for C, first in combos:
            masks = [_alloc(eng, n, compact) for _ in range(C)]
            eng.cohort_masks_dev(it, first, C, n, J, masks, compact=compact)
            for c in range(C):
                want = _words((streams[first + c] - streams[first + c + 1]) & M, L)
                _same(_get(eng, masks[c], n, compact), want, b, compact, J, n, C, first, c)


def test_the_mask_chain_is_what_prepare_encrypt_leaves(E):
    """mask[c] = add - minus of the vectors flashe_prepare_encrypt leaves in the ctx for that idx (prepared_download)."""
    b, J, n, it = 20, 16, _chain_length(20, 16, 3001), 4
    eng = E.Engine(KEY, b, device=0)
    masks = [_alloc(eng, n, True) for _ in range(3)]
    eng.cohort_masks_dev(it, 5, 3, n, J, masks, compact=True)
    for c in range(3):
        eng.prepare_encrypt(it, 5 + c, E.SCHEME_DOUBLE, n, J)
        add, minus = (eng.prepared_download(eng.PREPARED_ENCRYPT, part).reshape(-1).copy() for part in ("add", "minus"))
        want = (add - minus) & np.uint64((1 << b) - 1)
        _same(_get(eng, masks[c], n, True), want, "client", c)
        eng.prepared_discard(eng.PREPARED_ENCRYPT)


def test_the_compact_mask_chain_refuses_what_check_u32_refuses(E):
    eng = E.Engine(KEY, 64, device=0)
    d = eng.alloc(4096)
    for args in ((eng, 0, 0, 1, 100, 16), ):
        with pytest.raises(E.FlasheError) as ei:
            args[0].cohort_masks_dev(*args[1:], [d], compact=True)
        assert ei.value.code == -22
    eng = E.Engine(KEY, 20, device=0)
    for first, C, n, J, vec in ((0, 1, 100, 0, d), (2 ** 32 - 2, 2, 100, 16, d), (0, 1, 100, 16, d.ptr + 2)):
        with pytest.raises(E.FlasheError) as ei:
            eng.cohort_masks_dev(0, first, C, n, J, [vec] * C, compact=True)
        assert ei.value.code == -22, (first, C, n, J)
    eng.cohort_masks_dev(0, 0, 1, 0, 16, [d], compact=True)          # an empty vector: OK, nothing launched


# ------------------------------------------------------------------------------------------------ 2. the online launch
class _Cohort:
    """The shared rows, every client's sources (float32 and float64 rows alternate) and draws of an un-batched cohort, and per client the
    fused step's ciphertext (quantize_encrypt_model_dev, double mask) and its plaintext (the quantiser alone)."""

    def __init__(self, E, eng, bits, J, C, sizes, it=3, first_idx=5, alias=False, refs=True):
        from flashe_amd import _lib
        self.eng, self.bits, self.J, self.C, self.it, self.first_idx, self.sizes = eng, bits, J, C, it, first_idx, sizes
        self.n = n = sum(sizes)
        L = eng.limbs
        starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(int).tolist()
        codes = [_lib.TENSOR_F64 if li % 2 else _lib.TENSOR_F32 for li in range(len(sizes))]
        self.rows = [(starts[li], None, ALPHAS[li], 0.0, codes[li], 0) for li in range(len(sizes))]
        u = np.random.Generator(np.random.PCG64(eng.int_bits * 1000 + J * 10 + C)).random(max(C * n, 1))
        u[::5] = 0.0
        u[1::5] = 1.0 - 2.0 ** -53
        self.du = eng.upload(u)
        self.srcs, self.dts, self.keep, self.want, self.pts = [], [], [], [], []
        for c in range(C):
            if alias and c:
                self.srcs.append(self.srcs[0])
                self.dts.append(self.dts[0])
            else:
                xs = [_values(np.float64 if li % 2 else np.float32, ALPHAS[li], size, 100 * c + li) for li, size in enumerate(sizes)]
                ds = [eng.upload(x) if x.size else eng.alloc(16) for x in xs]
                self.keep += ds
                self.srcs.append([d.ptr for d in ds])
                self.dts.append(list(codes))
            if not refs or (alias and c > 1 and c < C - 1):
                continue                                                 # (aliased sources: the first two and the last client are checked)
            draws = E.DeviceBufferView(self.du, 8 * c * n, 8 * n)
            table = [(starts[li], self.srcs[c][li], ALPHAS[li], bool(li % 2)) for li, size in enumerate(sizes) if size]
            ref = eng.alloc_vec(n)
            eng.quantize_encrypt_model_dev(it, first_idx + c, E.SCHEME_DOUBLE, n, J, 0, n, table, bits, draws, ref)
            self.want.append((c, ref.download(np.uint64, n * L).copy()))
            ttab = [(starts[li], self.srcs[c][li], ALPHAS[li], 0.0, codes[li], 0) for li in range(len(sizes))]
            pt = eng.alloc_vec(n)
            eng.quantize_batch_tensors_dev(ttab, n, bits, eng.int_bits, draws.ptr, n, pt)
            self.pts.append((c, pt.download(np.uint64, n * L).copy()))

    def chain_masks(self, compact):
        masks = [_alloc(self.eng, self.n, compact) for _ in range(self.C)]
        self.eng.cohort_masks_dev(self.it, self.first_idx, self.C, self.n, self.J, masks, compact=compact)
        return masks

    def run(self, masks, compact, with_sum=True):
        eng, n = self.eng, self.n
        cts, dsum = [_alloc(eng, n, compact) for _ in range(self.C)], _alloc(eng, n, compact)
        ok = eng.quantize_combine_cohort_dev(n, self.rows, self.srcs, self.dts, self.bits, self.du, masks, cts, dsum if with_sum else None,
                                             compact=compact)
        assert ok is True
        return [_get(eng, d, n, compact) for d in cts], _get(eng, dsum, n, compact)


ONLINE = [(128, 16, False), (64, 16, False), (20, 16, False), (16, 12, True), (20, 16, True), (23, 16, True), (24, 16, True), (32, 24, True)]


@pytest.mark.parametrize("head", HEADS, ids=["issue-sizes", "no-start-on-4"])
@pytest.mark.parametrize("b,bits,compact", ONLINE)
def test_the_online_launch_with_the_chains_masks_is_every_clients_fused_step(E, b, bits, compact, head):
    """C = 3 (a group of two and a single) and C = 10."""
    eng = E.Engine(KEY, b, device=0)
    for C in (3, 10):
        co = _Cohort(E, eng, bits, 16, C, _sizes(head))
        got, gsum = co.run(co.chain_masks(compact), compact)
        for c, want in co.want:
            _same(got[c], want, b, compact, C, "client", c)
        _same(gsum, _host_sum(got, b, eng.limbs), b, compact, C, "sum")


@pytest.mark.parametrize("b,num_clients,field_bits,C", [(120, 10, None, 10), (120, 10, 24, 3), (128, 2, None, 2), (64, 4, None, 3), (120, 4, 60, 3), (128, 2, 128, 2)])
def test_the_batched_online_launch_is_every_clients_quantise_batch_encrypt(E, b, num_clients, field_bits, C):
    """bs 6, 5 and 7 (whole elements in 16-byte runs) and bs 3 at one limb, 2 and 1 (the run-time size); the layers include one of a single
    value, an empty one and sizes that are 1 and bs - 1 mod bs (test_gpu_cohort_batch._elems_to_sizes)."""
    from test_gpu_cohort_batch import _elems_to_sizes, _field_bits
    eng = E.Engine(KEY, b, device=0)
    L, n_elems, it, first_idx = eng.limbs, 6000, 3, 5
    fb = field_bits or _field_bits(num_clients)
    bs = b // fb
    assert bs == {(120, None): 6, (120, 24): 5, (128, None): 7, (64, None): 3, (120, 60): 2, (128, 128): 1}[(b, field_bits)]
    sizes = _elems_to_sizes(bs, n_elems) if bs > 1 else [1, 0, 100, 27, 640, 5001, 231]
    if L == 2:
        case = _Case(E, eng, b, num_clients, C, n_elems, first_idx=first_idx, it=it, field_bits=fb, sizes=sizes)
        rows, srcs, dts, du, n, want, keep = case.rows, case.srcs, case.dts, case.du, case.n, case.want, case.keep
    else:
        # (the one-limb batched step: _Case downloads two limbs per element, so the references are made here)
        co = _Cohort(E, eng, 16, 16, C, sizes, refs=False)
        rows, srcs, dts, du, n, want, keep = co.rows, co.srcs, co.dts, co.du, co.n, [], co.keep
        for c in range(C):
            table = [(r[0], srcs[c][li], r[2], 0.0, r[4], 0) for li, r in enumerate(rows)]
            pt, ref = eng.alloc_vec(n_elems), eng.alloc_vec(n_elems)
            eng.quantize_batch_tensors_dev(table, n, 16, fb, du.ptr + 8 * c * n, n_elems, pt)
            eng.encrypt_dev(it, first_idx + c, E.SCHEME_DOUBLE, n_elems, 16, pt, 1, ref)
            want.append(ref.download(np.uint64, n_elems).copy())
    masks = [_alloc(eng, n_elems, False) for _ in range(C)]
    eng.cohort_masks_dev(it, first_idx, C, n_elems, 16, masks)
    cts, dsum = [_alloc(eng, n_elems, False) for _ in range(C)], _alloc(eng, n_elems, False)
    assert eng.quantize_combine_cohort_dev(n, rows, srcs, dts, 16, du, masks, cts, dsum, batch=(n_elems, fb)) is True
    got = [_get(eng, d, n_elems, False) for d in cts]
    for c in range(C):
        _same(got[c], want[c], b, bs, "client", c)
    _same(_get(eng, dsum, n_elems, False), _host_sum(got, b, L), b, bs, "sum")
    del keep


# ------------------------------------------------------------------------------------------------ 3. carry and wrap edges, hand-made masks
def _mask_vectors(eng, n, compact, value):
    L = eng.limbs
    if compact:
        return eng.upload(np.full(n, value, dtype=np.uint32))
    a = np.zeros((n, L), dtype=np.uint64)
    a[:, 0] = value & (2 ** 64 - 1)
    if L == 2:
        a[:, 1] = value >> 64
    return eng.upload(a)


@pytest.mark.parametrize("b,bits,compact,ones", [(128, 16, False, 2 ** 64 - 1), (120, 16, False, 2 ** 64 - 1), (128, 16, False, 2 ** 128 - 1), (20, 16, False, 2 ** 20 - 1),
                                                  (20, 16, True, 2 ** 20 - 1), (23, 16, True, 2 ** 23 - 1), (23, 16, False, 2 ** 23 - 1), (32, 24, True, 2 ** 32 - 1)])
def test_all_ones_and_all_zero_masks_against_host_arithmetic(E, b, bits, compact, ones):
    """All-ones masks: a low limb of ones carries into limb 1 for every non-zero plaintext (int_bits 128 / 120), 2^b - 1 wraps every value
    and makes a sum that must be reduced (20 / 23; at 32 the uint32 wraps by itself).  All-zero masks: the plain quantisation."""
    eng = E.Engine(KEY, b, device=0)
    L, C = eng.limbs, 3
    co = _Cohort(E, eng, bits, 16, C, _sizes(HEADS[1]))
    M = (1 << b) - 1
    assert any((p != 0).any() for _c, p in co.pts)
    for value in (ones, 0):
        masks = [_mask_vectors(eng, co.n, compact, value)] * C
        got, gsum = co.run(masks, compact)
        want = [(_ints(p, L) + value) & M for _c, p in co.pts]
        for c in range(C):
            _same(got[c], _words(want[c], L), b, compact, hex(value), "client", c)
        _same(gsum, _words(sum(want) & M, L), b, compact, hex(value), "sum")
        if value == 0:
            for c, p in co.pts:
                _same(got[c], p, b, compact, "zero mask: the plain quantisation", c)


# ------------------------------------------------------------------------------------------------ 4. shares, null sum, empty model
@pytest.mark.parametrize("b,bits,compact", [(128, 16, False), (20, 16, True)])
def test_more_clients_than_an_argument_block_carries(E, b, bits, compact):
    """C = 130 clients that all read client 0's model (their draws and masks differ): every ciphertext and the sum."""
    eng = E.Engine(KEY, b, device=0)
    C, n = 130, 3001
    co = _Cohort(E, eng, bits, 16, C, _sizes([1, 6, 0, 1001, 256 * 3 + 91], n), alias=True, first_idx=0)
    got, gsum = co.run(co.chain_masks(compact), compact)
    assert [c for c, _w in co.want] == [0, 1, 129]
    for c, want in co.want:
        _same(got[c], want, b, compact, "client", c)
    # the other clients: (plaintext + the chain's mask), the plaintext from the quantiser alone with that client's draws
    L, M = eng.limbs, (1 << b) - 1
    assert not any((g == got[0]).all() for g in got[1:])
    _same(gsum, _host_sum(got, b, L), b, compact, "sum")
    streams = []
    for idx in (64, 65):
        d = eng.alloc_vec(n)
        eng.mask_dev(co.it, [idx], n, 16, d)
        streams.append(_ints(d.download(np.uint64, n * L), L))
    table = [(r[0], co.srcs[64][li], r[2], 0.0, r[4], 0) for li, r in enumerate(co.rows)]
    pt = eng.alloc_vec(n)
    eng.quantize_batch_tensors_dev(table, n, bits, b, co.du.ptr + 8 * 64 * n, n, pt)
    _same(got[64], _words((_ints(pt.download(np.uint64, n * L), L) + streams[0] - streams[1]) & M, L), b, compact, "client 64")


@pytest.mark.parametrize("b,bits,compact", [(128, 16, False), (20, 16, False), (20, 16, True)])
def test_a_null_sum_and_an_empty_model(E, b, bits, compact):
    from flashe_amd import _lib
    eng = E.Engine(KEY, b, device=0)
    co = _Cohort(E, eng, bits, 16, 3, _sizes([1, 7, 0, 1001, 256 * 3 + 91], 4099))
    masks = co.chain_masks(compact)
    got, gsum = co.run(masks, compact, with_sum=False)
    for c, want in co.want:
        _same(got[c], want, b, compact, "client", c)
    poison = 0xA5A5A5A5 if compact else 0xA5A5A5A5A5A5A5A5
    assert (gsum == np.uint64(poison)).all()
    # n = 0: FLASHE_OK, nothing launched, nothing written -- with layers that are all empty, with and without a sum
    d, d2 = _alloc(eng, 4, compact), _alloc(eng, 4, compact)
    rows = [(0, None, 1.0, 0.0, _lib.TENSOR_F32, 0), (0, None, 1.0, 0.0, _lib.TENSOR_F64, 0)]
    none, codes = [[None, None]] * 2, [[_lib.TENSOR_F32, _lib.TENSOR_F64]] * 2
    for s in (d2, None):
        assert eng.quantize_combine_cohort_dev(0, rows, none, codes, bits, None, [d, d], [d, d], s, compact=compact) is True
    if not compact:
        assert eng.quantize_combine_cohort_dev(0, rows, none, codes, bits, None, [d, d], [d, d], d2, batch=(0, b)) is True
    assert all((_get(eng, v, 4, compact) == np.uint64(poison)).all() for v in (d, d2))


# ------------------------------------------------------------------------------------------------ 5. refusals
def _refused(E, call):
    with pytest.raises(E.FlasheError) as ei:
        call()
    assert ei.value.code == -22, ei.value
    return str(ei.value)


@pytest.mark.parametrize("b,compact", [(128, False), (20, False), (20, True)])
def test_refusals(E, b, compact):
    """FLASHE_EINVAL with nothing written: a sum that is a mask, an output or a source; a float64 source under a float32 row; misaligned
    vectors; null vectors; a table that does not describe n; element_bits out of range."""
    from flashe_amd import _lib
    eng = E.Engine(KEY, b, device=0)
    n, C, eb = 1000, 2, _elem_bytes(eng, compact)
    x = [eng.upload(np.zeros(n, np.float32)) for _ in range(C)]
    x64 = eng.upload(np.zeros(n, np.float64))
    u = eng.upload(np.zeros(C * n))
    masks = [_alloc(eng, n + 4, compact, fill=0) for _ in range(C)]
    cts = [_alloc(eng, n + 4, compact) for _ in range(C)]
    dsum = _alloc(eng, n + 4, compact)
    rows = [(0, None, 1.0, 0.0, _lib.TENSOR_F32, 0)]
    srcs, dts = [[d.ptr] for d in x], [[_lib.TENSOR_F32]] * C

    def call(n=n, rows=rows, srcs=srcs, dts=dts, bits=16, u=u, masks=masks, cts=cts, dsum=dsum):
        return lambda: eng.quantize_combine_cohort_dev(n, rows, srcs, dts, bits, u, masks, cts, dsum, compact=compact)

    assert "alias" in _refused(E, call(dsum=masks[1]))
    assert "alias" in _refused(E, call(dsum=cts[0]))
    assert "alias" in _refused(E, call(dsum=x[1]))
    assert "float64 source under a float32 row" in _refused(E, call(srcs=[[x[0].ptr], [x64.ptr]], dts=[[_lib.TENSOR_F32], [_lib.TENSOR_F64]]))
    half = eb // 2
    assert "aligned" in _refused(E, call(cts=[cts[0], cts[1].ptr + half]))
    assert "aligned" in _refused(E, call(masks=[masks[0].ptr + half, masks[1]]))
    assert "aligned" in _refused(E, call(dsum=dsum.ptr + half))
    assert "aligned" in _refused(E, call(u=u.ptr + 4))
    assert "misaligned" in _refused(E, call(srcs=[[x[0].ptr + 2], [x[1].ptr]]))
    _refused(E, call(cts=[cts[0], None]))
    _refused(E, call(masks=[None, masks[1]]))
    _refused(E, call(u=None))
    _refused(E, call(srcs=[[x[0].ptr], [None]]))
    _refused(E, call(rows=[(0, None, 1.0, 0.0, _lib.TENSOR_F32, 0), (n + 1, None, 1.0, 0.0, _lib.TENSOR_F32, 0)], srcs=[[x[0].ptr] * 2] * 2, dts=[[_lib.TENSOR_F32] * 2] * 2))
    _refused(E, call(rows=[(0, None, 0.0, 0.0, _lib.TENSOR_F32, 0)]))
    _refused(E, call(rows=[(0, None, 1.0, 0.0, _lib.TENSOR_BF16, 0)]))
    _refused(E, call(bits=0))
    _refused(E, call(bits=min(b, 62) + 1))
    with pytest.raises(E.FlasheError) as ei:
        eng.quantize_combine_cohort_dev(n, rows, [], [], 16, u, [], [], dsum, compact=compact)
    assert ei.value.code == -22
    poison = 0xA5A5A5A5 if compact else 0xA5A5A5A5A5A5A5A5
    assert all((_get(eng, d, n, compact) == np.uint64(poison)).all() for d in cts + [dsum])
    # and the call they were derived from is taken
    assert call()() is True
    if not compact:
        # the batched form: n_elems that is not what the layers batch into, field_bits outside element_bits .. int_bits
        fb = 20 if b > 64 else 10
        bits = 16 if b > 64 else 8
        bs = b // fb
        n_elems = -(-n // bs)
        bcall = lambda ne, f, eb_=bits: (lambda: eng.quantize_combine_cohort_dev(n, rows, srcs, dts, eb_, u, masks, cts, dsum, batch=(ne, f)))       # noqa: E731
        assert "batch into" in _refused(E, bcall(n_elems + 1, fb))
        assert "batch into" in _refused(E, bcall(n_elems - 1, fb))
        _refused(E, bcall(n_elems, bits - 1))
        _refused(E, bcall(n_elems, b + 1))
        assert bcall(n_elems, fb)() is True


def test_the_compact_form_needs_a_compact_ctx(E):
    """int_bits > 32: FLASHE_EINVAL."""
    from flashe_amd import _lib
    eng = E.Engine(KEY, 64, device=0)
    n = 100
    x, u = eng.upload(np.zeros(n, np.float32)), eng.upload(np.zeros(n))
    m, ct = _alloc(eng, n, True, fill=0), _alloc(eng, n, True)
    _refused(E, lambda: eng.quantize_combine_cohort_dev(n, [(0, None, 1.0, 0.0, _lib.TENSOR_F32, 0)], [[x.ptr]], [[_lib.TENSOR_F32]], 16, u, [m], [ct], None, compact=True))
