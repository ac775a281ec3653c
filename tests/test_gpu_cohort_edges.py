"""GPU: the fused cohort launches -- the compact chain (flashe_quantize_encrypt_cohort_u32_dev), the batched chain
(flashe_quantize_batch_encrypt_cohort_dev), the sparse compact chain (flashe_quantize_encrypt_sparse_cohort_dev), the prepared online step
(flashe_quantize_combine_cohort_dev / _u32_dev / flashe_quantize_batch_combine_cohort_dev) and the batched back end over caller-held masks
(flashe_combine_unbatch_unquantize_model_dev) -- against the NumPy / Python-int reference of tests/codec_ref.py composed with the oracle's
cipher, where the quantiser leaves its nominal range: q == 2^bits (x >= alpha under the draw 1 - 2^-53) and q == 2^bits + 1 (float32 from 25
bits on) going into a uint32 cast at element_bits == int_bits, into a batch field with field_bits == element_bits (the carry runs into
the neighbouring field and out of the top of a 120-bit element) and into the running sum of the prepared kernels; alphas of 1e-30 and
1e30, +-inf, subnormals, +-0; vectors that are element-aligned but not 16-byte aligned.

Every case is built on the CPU (the builders below are what tests/test_codec_edges_host.py checks without a GPU) and holds the conditions
of codec_ref.check_cohort_case on the reference alone.  Outputs are poisoned with 0xA5, one guard element behind each must stay so, and
every launch must be taken.  Integers are compared exactly, floats as bytes: no tolerance anywhere."""
import numpy as np
import pytest

import codec_ref as R
from test_gpu_cohort_batch import _elems_to_sizes
from test_gpu_cohort_compact import _length
from test_gpu_cohort_prepared import _chain_length
from test_gpu_sparse_cohort_front_end import LAST_DRAW, SHAPES

pytestmark = pytest.mark.gpu

KEY = bytes(range(32))
C, IT, FIRST = 3, 3, 5                                   # a group of two and a single client in the prepared kernels; an odd chain length
POISON8 = np.uint64(0xA5A5A5A5A5A5A5A5)


@pytest.fixture(scope="module")
def E():
    from flashe_amd import engine
    return engine


# ================================================================================================ the cases, built on the CPU
# ------------------------------------------------------------------------------------------------ compact chain
COMPACT = [(16, 16), (20, 20), (24, 24), (32, 32), (32, 25), (20, 1)]      # int_bits, element_bits
COMPACT_J = (1, 16)


def compact_length(b, J):
    """An odd length a few hundred values past the compact launch's admission on two CUs whose chunks end in partial AES blocks
    (test_gpu_cohort_compact._length): odd, so that client 1's draws begin at an address that is 8 mod 16."""
    for extra in range(300, 600):
        n = _length(b, J, extra=extra)
        if n % 2:
            return n
    raise AssertionError((b, J))


def compact_spec(n):
    """storage, alpha, shift, wide, loop64, size: both compute types read in place, a float16 and a bfloat16 staged row, a SHIFT row, a
    LOOP_F64 row; 1e30 on the float64 row only; every size odd."""
    head = [("float32", 1e-30, None, False, False, 10007), ("float64", 1e30, None, False, False, 4099), ("float16", 0.1, None, False, False, 1019),
            ("bfloat16", 1.0, None, False, False, 3), ("float32", 0.1, 0.0625, False, False, 777), ("float32", 1.0, None, False, True, 2049)]
    rest = n - sum(s[5] for s in head)
    assert rest % 2 == 1 and rest > 0
    return head + [("float32", 1.0, None, False, False, rest)]


def compact_case(b, bits, J):
    n = compact_length(b, J)
    model = R.cohort_model(compact_spec(n), C, seed=b + bits + J)
    return model, R.check_cohort_case(model, bits)


# ------------------------------------------------------------------------------------------------ batched chain and batched prepared step
BATCH_CHAIN = [(120, 24, 24), (120, 20, 20), (128, 18, 18), (128, 25, 25), (120, 20, 16)]      # int_bits, field_bits, element_bits: bs 5, 6, 7, 5, 6
BATCH_PREPARED = BATCH_CHAIN + [(64, 21, 21), (120, 60, 60), (120, 62, 62)]                     # and the run-time sizes 3, 2, 1
CHAIN_ELEMS = 16129 + 334                               # past the wide chain's admission on two CUs (cohort_admission_length(2))
PREPARED_ELEMS = 12001


def _carry_row(bs, start):
    """The size of a float32 row of alpha 1.0 that begins at value `start` and whose padded last element overflows on the reference:
    layer_fill repeats the plane with an odd period P, the plane's values 2, 4, 8 and 15 are alpha, its upper neighbour, +inf and the largest float, and value
    j of client 0 meets the draw 1 - 2^-53 where j % 4 == 1.  So: a size s with s % bs >= 2 (the last element holds a value before
    the row's last, which is -alpha), (s - 2) % P in (2, 4, 8, 15) and (start + s - 2) % 4 == 1."""
    P = len(R.edge_plane(np.float32, 1.0, 1500))
    P -= 1 - P % 2
    for k in range(1, 7):
        for i in (2, 4, 8, 15):
            s = k * P + i + 2
            if s % bs >= 2 and (start + s - 2) % 4 == 1:
                return s
    raise AssertionError((bs, start))


def batch_spec(bs, n_elems):
    """_elems_to_sizes' rows (sizes = 0, 1 and bs - 1 mod bs, a single value, an empty row) over both compute types, a staged row; from
    bs 3 on one more row in front of the last, sized by _carry_row."""
    kinds = [("float32", 1.0), ("float64", 0.1), ("float32", 0.1), ("float64", 1.0), ("bfloat16", 1.0), ("float64", 1e-30), ("float32", 1.0)]
    if bs == 1:
        sizes = [1, 0, 100, 27, 640, 5001, n_elems - 5769]
    else:
        carry = _carry_row(bs, 5766 * bs + 3) if bs > 2 else 0             # (5766 bs + 3: the values of _elems_to_sizes' first six rows)
        sizes = _elems_to_sizes(bs, n_elems - -(-carry // bs))
        assert sum(sizes[:6]) == 5766 * bs + 3
        if carry:
            sizes.insert(6, carry)
            kinds.insert(6, ("float32", 1.0))
    return [(st, alpha, None, False, False, size) for (st, alpha), size in zip(kinds, sizes)]


def batch_case(b, fb, eb, n_elems):
    """-> model, per-client plaintexts, per-client batched elements (mod 2^b), the field overflows of the reference."""
    bs = b // fb
    model = R.cohort_model(batch_spec(bs, n_elems), C, seed=b + fb)
    pts = R.check_cohort_case(model, eb)
    batched = R.cohort_batched(model, eb, b, fb)
    assert all(len(t) == n_elems for t in batched)
    over = R.cohort_field_overflows(model, eb, b, fb)
    if fb == eb:
        # the carry cases: a field that overflows in a row's first element, in a row's padded last element and -- where the fields
        # fill the element, 5 x 24 and 6 x 20 at 120 bits -- in slot 0: the carry leaves the element at bit 120
        assert any(e == 0 for _c, _l, e, _s, _ne, _size in over), "no overflow in a row's first element"
        # (bs <= 2: a padded last element holds the row's last value alone, which layer_fill makes -alpha)
        assert any(e == ne - 1 and size % bs for _c, _l, e, _s, ne, size in over) or bs <= 2, "no overflow in a row's padded last element"
        if bs * fb == b:
            assert any(s == 0 for _c, _l, _e, s, _ne, _size in over), "no carry out of the top field"
    else:
        assert not over
    return model, pts, batched, over


# ------------------------------------------------------------------------------------------------ sparse compact chain
SPARSE_WIDTHS = (16, 20, 23, 24, 32)
SPARSE = [(b, eb, shape) for b in SPARSE_WIDTHS for eb in sorted({16, b}) for shape in ("partial-blocks", "tiles")]
ZZZ = (0.0, 1.0, -1.0, 0.3, -7.0, 2.5)
TAIL_DRAWS = (0.0, LAST_DRAW, 0.5)


def sparse_case(b, eb, shape):
    """The existing file's shape (K, n_jobs, layer sizes) for C clients; every source class and one LOOP_F64 row, cycled as there.
    -> model, plaintexts, the draws in the launch's layout (client c's K draws and its 'zzz' draw at c * (K + 1)), the zzz values, the
    quantised zeros of the reference."""
    K, n_jobs, _C, sizes = SHAPES[shape]
    kinds = [("float32", 1.0, False), ("float64", 0.1, False), ("float16", 1.0, False), ("bfloat16", 0.1, False), ("float32", 1e-30, True), ("float32", 0.1, False)]
    spec = [(kinds[i % 6][0], kinds[i % 6][1], None, False, kinds[i % 6][2], size) for i, size in enumerate(sizes)]
    model = R.cohort_model(spec, C, seed=b + eb)
    pts = R.check_cohort_case(model, eb)
    u = np.zeros(C * (K + 1))
    zzz = [ZZZ[c % 6] for c in range(C)]
    zeros = []
    zt = np.float64 if b % 2 == 0 else np.float32
    for c in range(C):
        u[c * (K + 1):c * (K + 1) + K] = model.u[c * K:(c + 1) * K]
        u[c * (K + 1) + K] = TAIL_DRAWS[c % 3]
        zeros.append(int(R.ref_quantize(np.array([zzz[c]], dtype=zt), 1.0, eb, [TAIL_DRAWS[c % 3]])[0]))
    assert zeros[1] == 1 << eb                           # 'zzz' = alpha under the draw 1 - 2^-53: a quantised zero of 2^int_bits where eb == int_bits
    return model, pts, u, zzz, zeros, K, n_jobs


# ------------------------------------------------------------------------------------------------ prepared step, un-batched
PREPARED = [(16, 16, True), (32, 32, True), (32, 25, True), (20, 20, False), (64, 33, False), (128, 24, False), (120, 62, False)]   # int_bits, element_bits, compact
PREPARED_TYPES = [(32, 32, True), (64, 33, False), (128, 24, False)]       # one case per element type: uint32, uint64, u128
PREPARED_J = 16


def prepared_spec(n):
    head = [("float32", 1.0, None, False, False, 1), ("float64", 1e30, None, False, False, 6), ("float16", 0.1, None, False, False, 1019),
            ("float32", 1e-30, None, False, False, 1777), ("bfloat16", 1.0, 0.25, True, False, 3), ("float32", 0.1, None, False, True, 801)]
    rest = n - sum(s[5] for s in head)
    assert rest > 0
    return head + [("float32", 1.0, None, False, False, rest)]


def prepared_length(b):
    """A length whose PREPARED_J chunks end in partial AES blocks, for the mask chain in front of the step."""
    return _chain_length(b, PREPARED_J, 6001)


def prepared_case(b, bits, n=None):
    n = prepared_length(b) if n is None else n
    model = R.cohort_model(prepared_spec(n), C, seed=b + bits + n)
    return model, R.check_cohort_case(model, bits)


# ------------------------------------------------------------------------------------------------ batched back end
BACK_END = [(120, 20, 16, 10), (128, 18, 16, 3)]         # int_bits, field_bits, element_bits, num_clients: bs 6 and 7


def back_end_case(b, fb, eb, nc):
    """Aggregates whose fields hold sum_plane's values and the all-ones field; rows with padded last elements.  -> layers, items, floats"""
    bs = b // fb
    sizes = [1, 0, 100 * bs, 26 * bs + 1, 639 * bs + bs - 1, 200 * bs + 2]
    alphas = [1.0, 0.1, 1e-30, 1e30, 8.17121, 3e-3]
    plane = R.sum_plane(eb, nc, int_bits=min(fb, 64), n_random=1500)
    items, want = [], []
    for i, (size, alpha) in enumerate(zip(sizes, alphas)):
        vals = np.resize(np.array(plane[i:] + [(1 << fb) - 1], dtype=object), size).tolist()
        row = R.ref_batch(vals, b, fb)
        assert R.ref_unbatch(row, b, fb)[:size] == vals
        items += row
        want.append(R.ref_unquantize(vals, alpha, eb, nc))
    return [(s, None, a, False) for s, a in zip(sizes, alphas)], items, np.concatenate(want)


# ================================================================================================ device helpers
def _out(E, eng, n, elem_bytes, off=0):
    """A poisoned vector of n elements and one guard element behind them, `off` bytes past a 16-byte boundary."""
    d = eng.alloc(elem_bytes * (n + 1) + 32)
    eng.memset_dev(d, 0xA5, d.nbytes)
    assert d.ptr % 16 == 0
    return E.DeviceBufferView(d, off, elem_bytes * (n + 1))


def _get(v, n, elem_bytes):
    """-> the n elements as Python ints (object array), and whether the guard element still holds the poison"""
    if elem_bytes == 4:
        a = v.download(np.uint32, n + 1)
        return a[:n].astype(np.uint64).astype(object), int(a[n]) == 0xA5A5A5A5
    a = v.download(np.uint64, (n + 1) * elem_bytes // 8)
    guard = bool((a[n * elem_bytes // 8:] == POISON8).all())
    a = a[:n * elem_bytes // 8]
    if elem_bytes == 8:
        return a.astype(object), guard
    a = a.reshape(n, 2)
    return a[:, 0].astype(object) + (a[:, 1].astype(object) << 64), guard


def _ints(limbs):
    """an oracle result [n, L] as Python ints"""
    return np.array(R.from_limbs(limbs) if limbs.shape[1] > 1 else [int(v) for v in limbs[:, 0]], dtype=object)


def _same(got, want, *what):
    got, want = np.asarray(got, dtype=object), np.asarray(want, dtype=object)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad[:6], [hex(int(v)) for v in got[bad[:6]]], [hex(int(v)) for v in want[bad[:6]]], bad.size)


def _sources(eng, model, odd_client=None):
    """Every client's rows in HBM; client `odd_client`'s float32 sources 4 bytes past a 16-byte boundary."""
    keep, srcs = [], []
    for c in range(model.C):
        row = []
        for li, raw in enumerate(model.storage[c]):
            off = 4 if c == odd_client and model.dts[li] == R.F32 else 0
            d = eng.alloc(raw.nbytes + 32)
            assert d.ptr % 16 == 0
            d.upload_at(off, raw)
            keep.append(d)
            row.append(d.ptr + off)
        srcs.append(row)
    return srcs, [list(model.dts) for _ in range(model.C)], keep


def _limbs(ints, b):
    return R.to_limbs(ints, 2 if b > 64 else 1)


def _want_cts(oracle, pts, b, J, scheme="double", idx=None):
    """Every client's oracle ciphertext of its plaintext mod 2^b, and the oracle's sum of them."""
    M = (1 << b) - 1
    cts = [oracle.encrypt(KEY, IT, (FIRST + c) if idx is None else idx[c], scheme, J, b, _limbs([int(v) & M for v in p], b)) for c, p in enumerate(pts)]
    return [_ints(ct) for ct in cts], _ints(oracle.aggregate_elem(cts, b))


# ================================================================================================ 2. the four encrypt launches
@pytest.mark.parametrize("J", COMPACT_J)
@pytest.mark.parametrize("b,bits", COMPACT)
def test_compact_chain_against_numpy_and_the_oracle(E, oracle, b, bits, J):
    """q == 2^bits and 2^bits + 1 into the uint32 cast at element_bits == int_bits (a plaintext of 0 or 1 mod 2^b); at J = 16 client 1's
    float32 sources and its ciphertexts lie 4 bytes past a 16-byte boundary; the odd n puts its draws at 8 mod 16 everywhere."""
    model, pts = compact_case(b, bits, J)
    n = model.n
    eng = E.Engine(KEY, b, device=0)
    eng.set_cu_limit(2)
    odd = 1 if J == 16 else None
    srcs, dts, keep = _sources(eng, model, odd_client=odd)
    du = eng.upload(model.u)
    assert (du.ptr + 8 * n) % 16 == 8
    cts = [_out(E, eng, n, 4, off=4 if c == odd else 0) for c in range(C)]
    dsum = _out(E, eng, n, 4)
    assert eng.quantize_encrypt_cohort_u32_dev(IT, FIRST, n, J, model.rows, srcs, dts, bits, du, cts, dsum), "the compact cohort launch declined the shape"
    want, want_sum = _want_cts(oracle, pts, b, J)
    for c in range(C):
        got, guard = _get(cts[c], n, 4)
        _same(got, want[c], "compact chain", b, bits, J, "client", c)
        assert guard, ("a write behind the ciphertext", c)
    got, guard = _get(dsum, n, 4)
    _same(got, want_sum, "compact chain", b, bits, J, "sum")
    assert guard, "a write behind the sum"
    del keep


@pytest.mark.parametrize("b,fb,eb", BATCH_CHAIN)
def test_batched_chain_against_numpy_and_the_oracle(E, oracle, b, fb, eb):
    """field_bits == element_bits: q == 2^bits carries into the neighbouring field and, from slot 0 of a full 120-bit element, out of it."""
    model, _pts, batched, _over = batch_case(b, fb, eb, CHAIN_ELEMS)
    ne, J, M = CHAIN_ELEMS, 16, (1 << b) - 1
    eng = E.Engine(KEY, b, device=0)
    eng.set_cu_limit(2)
    srcs, dts, keep = _sources(eng, model)
    du = eng.upload(model.u)
    outs = [_out(E, eng, ne, 16) for _ in range(C + 2)]
    assert eng.quantize_batch_encrypt_cohort_dev(IT, FIRST, model.n, ne, J, model.rows, srcs, dts, eb, fb, du, outs[:C], outs[C], outs[C + 1]), \
        "the batched cohort launch declined the shape"
    want, want_sum = _want_cts(oracle, batched, b, J)
    for c in range(C):
        got, guard = _get(outs[c], ne, 16)
        _same(got, want[c], "batched chain", b, fb, eb, "client", c)
        assert guard, ("a write behind the ciphertext", c)
    gsum, guard = _get(outs[C], ne, 16)
    _same(gsum, want_sum, "batched chain", b, fb, eb, "sum")
    mask, guard2 = _get(outs[C + 1], ne, 16)
    assert guard and guard2, "a write behind the sum or the mask"
    plain = np.array([sum(t) & M for t in zip(*batched)], dtype=object)
    _same((gsum + mask) & M, plain, "batched chain", b, fb, eb, "sum + mask against the NumPy plaintexts")
    del keep


@pytest.mark.parametrize("b,eb,shape", SPARSE)
def test_sparse_compact_chain_against_numpy_and_the_oracle(E, oracle, b, eb, shape):
    """Every upload element against the oracle's SINGLE-mask encrypt of the NumPy plaintext; zeros_dev[c] and the trailing element against
    ref_quantize of the 'zzz' value, NOT reduced: the reference job strips the quantised zero before the encrypt and re-appends it in
    plain behind it (NOTES section 2), so a 'zzz' of alpha under the draw 1 - 2^-53 travels as 2^element_bits, which at element_bits ==
    int_bits is 2^int_bits in a one-limb element.  Client 1's upload lies 8 bytes past a 16-byte boundary."""
    model, pts, u, zzz, zeros, K, n_jobs = sparse_case(b, eb, shape)
    idx = list(range(FIRST, FIRST + C))
    eng = E.Engine(KEY, b, device=0)
    srcs, dts, keep = _sources(eng, model)
    du = eng.upload(u)
    ups = [_out(E, eng, K + 1, 8, off=8 if c == 1 else 0) for c in range(C)]
    dz = _out(E, eng, C, 8)
    assert eng.quantize_encrypt_sparse_cohort_dev(IT, idx, K, n_jobs, model.rows, srcs, dts, eb, du, K + 1, zzz, b % 2 == 0, ups, dz), \
        "the sparse cohort launch declined the shape"
    want, _sum = _want_cts(oracle, pts, b, n_jobs, scheme="single", idx=idx)
    gz, guard = _get(dz, C, 8)
    assert guard, "a write behind zeros_dev"
    _same(gz, zeros, "sparse chain", b, eb, shape, "zeros")
    for c in range(C):
        got, guard = _get(ups[c], K + 1, 8)
        _same(got[:K], want[c], "sparse chain", b, eb, shape, "client", c)
        assert int(got[K]) == zeros[c], ("the trailing element", c, hex(int(got[K])), hex(zeros[c]))
        assert guard, ("a write behind the upload", c)
    eng.close()
    del keep


# ------------------------------------------------------------------------------------------------ the prepared step
def _chain_masks(E, eng, n, compact, offs=0):
    """cohort_masks_dev's masks of the C clients (and as Python ints); offs: moved to vectors that many bytes past a 16-byte boundary"""
    eb = 4 if compact else 8 * eng.limbs
    masks = [_out(E, eng, n, eb) for _ in range(C)]
    eng.cohort_masks_dev(IT, FIRST, C, n, PREPARED_J, masks, compact=compact)
    if offs:
        moved = []
        for m in masks:
            raw = m.download(np.uint8, eb * n)
            d = _out(E, eng, n, eb, off=offs)
            d.parent.upload_at(offs, raw)
            moved.append(d)
        masks = moved
    return masks


def _run_prepared(E, eng, model, bits, masks, compact, n_out, batch=None, offs=0, odd_client=None):
    eb = 4 if compact else 8 * eng.limbs
    srcs, dts, keep = _sources(eng, model, odd_client=odd_client)
    du = eng.upload(model.u)
    cts, dsum = [_out(E, eng, n_out, eb, off=offs) for _ in range(C)], _out(E, eng, n_out, eb, off=offs)
    assert eng.quantize_combine_cohort_dev(model.n, model.rows, srcs, dts, bits, du, masks, cts, dsum, compact=compact, batch=batch) is True
    got = []
    for c, d in enumerate(cts + [dsum]):
        v, guard = _get(d, n_out, eb)
        assert guard, ("a write behind output", c)
        got.append(v)
    del keep
    return got[:C], got[C]


def _const_masks(eng, n, compact, value):
    if compact:
        return eng.upload(np.full(n, value, dtype=np.uint32))
    return eng.upload(R.to_limbs([value] * n, eng.limbs))


def _check_prepared(E, oracle, eng, model, pts, b, bits, compact, n_out, batch=None, offs=0, odd_client=None, ones=True):
    """pts: every client's plaintext elements (Python ints, un-batched values or batched elements).  The chain's masks: every ciphertext
    is the oracle's double-mask encrypt of the NumPy plaintext -- which ties cohort_masks_dev to the oracle too --, the sum the oracle's
    aggregate.  Hand-made masks of 2^b - 1: Python-int arithmetic on the NumPy plaintexts."""
    M = (1 << b) - 1
    got, gsum = _run_prepared(E, eng, model, bits, _chain_masks(E, eng, n_out, compact, offs), compact, n_out, batch, offs, odd_client)
    want, want_sum = _want_cts(oracle, pts, b, PREPARED_J)
    for c in range(C):
        _same(got[c], want[c], "prepared", b, bits, compact, batch, "client", c)
    _same(gsum, want_sum, "prepared", b, bits, compact, batch, "sum")
    if ones:
        got, gsum = _run_prepared(E, eng, model, bits, [_const_masks(eng, n_out, compact, M)] * C, compact, n_out, batch)
        want = [np.array([(int(v) + M) & M for v in p], dtype=object) for p in pts]
        for c in range(C):
            _same(got[c], want[c], "prepared, masks of 2^b - 1", b, bits, compact, batch, "client", c)
        _same(gsum, np.array([sum(t) & M for t in zip(*want)], dtype=object), "prepared, masks of 2^b - 1", b, bits, compact, batch, "sum")


@pytest.mark.parametrize("b,bits,compact", PREPARED)
def test_prepared_step_against_numpy_and_the_oracle(E, oracle, b, bits, compact):
    model, pts = prepared_case(b, bits)
    eng = E.Engine(KEY, b, device=0)
    _check_prepared(E, oracle, eng, model, pts, b, bits, compact, model.n)


@pytest.mark.parametrize("b,bits,compact", PREPARED_TYPES)
def test_prepared_step_one_element_past_a_16_byte_boundary(E, oracle, b, bits, compact):
    """Every mask, ciphertext and sum pointer one element (4, 8, 16 bytes) past a 16-byte boundary, client 1's float32 sources 4 bytes."""
    model, pts = prepared_case(b, bits)
    eng = E.Engine(KEY, b, device=0)
    _check_prepared(E, oracle, eng, model, pts, b, bits, compact, model.n, offs=4 if compact else 8 * eng.limbs, odd_client=1, ones=False)


@pytest.mark.parametrize("n", [4098, 4099, 4097])
@pytest.mark.parametrize("b,bits,compact", PREPARED_TYPES)
def test_prepared_step_tail_loop(E, oracle, b, bits, compact, n):
    """n = 1, 2 and 3 mod 4: the model's last run of four is partial and goes value by value."""
    assert n % 4 in (1, 2, 3)
    model, pts = prepared_case(b, bits, n)
    eng = E.Engine(KEY, b, device=0)
    _check_prepared(E, oracle, eng, model, pts, b, bits, compact, n, ones=False)


@pytest.mark.parametrize("b,fb,eb", BATCH_PREPARED)
def test_batched_prepared_step_against_numpy_and_the_oracle(E, oracle, b, fb, eb):
    """bs 5, 6 and 7 (compiled in) and 3, 2 and 1 (the run-time size) with field_bits == element_bits, and the shipped shape."""
    model, _pts, batched, _over = batch_case(b, fb, eb, PREPARED_ELEMS)
    eng = E.Engine(KEY, b, device=0)
    _check_prepared(E, oracle, eng, model, batched, b, eb, False, PREPARED_ELEMS, batch=(PREPARED_ELEMS, fb))


# ================================================================================================ 3. the batched back end
@pytest.mark.parametrize("b,fb,eb,nc", BACK_END)
def test_combine_unbatch_unquantize_against_python_ints(E, oracle, b, fb, eb, nc):
    """out = unquantise(unbatch((inp + add - minus) mod 2^b)) with add and minus masks of 0, of 2^b - 1 and of oracle streams, minus null
    and given, against ref_unbatch + ref_unquantize, as bytes."""
    layers, items, want = back_end_case(b, fb, eb, nc)
    ne, n, M, J = len(items), len(want), (1 << b) - 1, 16
    eng = E.Engine(KEY, b, device=0)
    streams = [R.from_limbs(oracle.mask(KEY, IT, idx, ne, J, b)) for idx in (nc, 0)]
    kinds = {"zero": [0] * ne, "ones": [M] * ne, "stream": streams[0], "stream0": streams[1]}
    out = eng.alloc(8 * (n + 1))
    for add, minus in [("zero", None), ("ones", None), ("stream", None), ("zero", "zero"), ("ones", "ones"), ("zero", "ones"), ("ones", "zero"),
                       ("stream", "stream0"), ("stream", "ones")]:
        A, S = kinds[add], (kinds[minus] if minus else [0] * ne)
        inp = [(t - a + s) & M for t, a, s in zip(items, A, S)]
        eng.memset_dev(out, 0xA5, 8 * (n + 1))
        eng.combine_unbatch_unquantize_model_dev(layers, eb, fb, nc, eng.upload(R.to_limbs(inp, 2)), eng.upload(R.to_limbs(A, 2)),
                                                 eng.upload(R.to_limbs(S, 2)) if minus else None, ne, out)
        got = out.download(np.float64, n + 1)
        assert got[n:].tobytes() == b"\xa5" * 8, "a write behind the floats"
        bad = np.flatnonzero(got[:n].view(np.uint64) != want.view(np.uint64))
        assert got[:n].tobytes() == want.tobytes(), (b, fb, add, minus, bad[:4], got[bad[:4]], want[bad[:4]], bad.size)
