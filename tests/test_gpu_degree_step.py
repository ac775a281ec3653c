"""GPU: the aggregator's degree scaling through the fused client step (flashe_stage_layers_dev, flashe_finish_layers_dev and the degree /
total_degree / last_round arguments of FlasheClient, FlasheCohort and FlasheSparseCohort).

The yardstick of every case is the reference's own sequence written out with NumPy on host copies (jzf_aggregator.py:676, :902-907):
`layer * degree` before the existing quantize_encrypt(normalize=True); the existing decrypt_unquantize, `/ (total / degree)`, the existing
unnormalize, `/ degree` and `last + w` after it, with the same np.random.seed.  Everything is compared as bytes, the statistics by their
hex form; there is no tolerance anywhere.  bfloat16 has no NumPy dtype: it travels as its uint16 bit patterns (round to nearest even of
the float32 value, upcast by a 16-bit shift)."""
import functools
import itertools
import operator
from fractions import Fraction

import numpy as np
import pytest

from flashe_amd import Engine, _lib

pytestmark = pytest.mark.gpu

KEY = bytes(range(32))
EINVAL = -22
F32, F64, F16, BF16 = _lib.TENSOR_F32, _lib.TENSOR_F64, _lib.TENSOR_F16, _lib.TENSOR_BF16
SC, SCW, SH, SHW, O64 = _lib.STAGE_SCALE, _lib.STAGE_SCALE_WIDE, _lib.STAGE_SHIFT, _lib.STAGE_SHIFT_WIDE, _lib.STAGE_OUT_F64
DT, FSH, DO, AL = _lib.FINISH_DIV_TOTAL, _lib.FINISH_SHIFT, _lib.FINISH_DIV_OWN, _lib.FINISH_ADD_LAST
SIZES = [1, 7, 8, 9, 127, 128, 129, 8193]            # 8,193: one value past a np.getbufsize() = 8,192 buffer of the statistics
SCALES = [5000.0, 37.0, 0.3]
DIVISORS = [(13700, 5000), (111, 37)]                # (total_degree, degree)
ES = {F32: 4, F64: 8, F16: 2, BF16: 2}
NPDT = {F32: np.float32, F64: np.float64, F16: np.float16, BF16: np.uint16}


# ---------------------------------------------------------------- bfloat16 as bit patterns
def bf16_bits(x32):
    """float32 -> bfloat16 bit patterns, round to nearest even (finite values)."""
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def stored(x64, code):
    """float64 values as a tensor of dtype `code` holds them (float64 -> float32 -> 16 bits), in its NumPy carrier dtype."""
    if code == F64:
        return np.asarray(x64, dtype=np.float64)
    x32 = np.asarray(x64, dtype=np.float64).astype(np.float32)
    return x32 if code == F32 else x32.astype(np.float16) if code == F16 else bf16_bits(x32)


def as_f32(a, code):
    """A stored 32- or 16-bit layer as the float32 array the step computes on (exact)."""
    return bf16_f32(a) if code == BF16 else np.asarray(a).astype(np.float32)


def layer_values(size, seed):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal(size) * 0.05


class Arena:
    """One device buffer handed out in slices: every slice starts `odd` elements behind a 16-byte boundary and has 16 poisoned bytes
    of guard behind it."""

    def __init__(self, eng, nbytes, poison=0xA5):
        self.buf, self.at, self.eng = eng.alloc(nbytes), 0, eng
        eng.memset_dev(self.buf, poison, nbytes)

    def take(self, size, es, odd):
        self.at = (self.at + 15) & ~15
        off = self.at + (es if odd else 0)
        self.at = off + size * es + 16
        assert self.at <= self.buf.nbytes
        return off

    def put(self, off, arr):
        self.buf.upload_at(off, arr)
        return self.buf.ptr + off

    def get(self, off, dtype, count):
        return self.buf.download_at(off, dtype, count)


@pytest.fixture(scope="module")
def eng():
    return Engine(KEY, 128)


# ---------------------------------------------------------------- the stage pass against NumPy
def stage_combos(code):
    """Every legal flag combination of a source stored as `code`."""
    if code == F64:
        return [O64 | a | b for a in (0, SC) for b in (0, SH)]
    out = [a | b | o for a in (0, SC) for b in (0, SH, SH | SHW) for o in (0, O64)]
    return out + [SC | SCW | O64 | b for b in (0, SH)]


def stage_ref(src, code, flags, scale, shift):
    """`layer * degree`, then normalize's in-place `+= shift`, then the widening of the loop dtype -- NumPy's own operations."""
    y = np.asarray(src, dtype=np.float64) if code == F64 else as_f32(src, code)
    if flags & SC:
        y = y * (np.float64(scale) if flags & SCW else float(scale))           # a Python float is weak, an np.float64 widens the layer
    if flags & SH:
        y = y.copy()
        y += np.float64(shift) if (flags & SHW) or y.dtype == np.float64 else float(shift)
    return y.astype(np.float64 if flags & O64 else np.float32)


def contracted(x, scale, shift, dtype):
    """round(x * scale + shift) with one rounding: what a fused multiply-add would store."""
    sc = Fraction(float(np.float32(scale))) if dtype == np.float32 else Fraction(float(scale))
    sh = Fraction(float(np.float32(shift))) if dtype == np.float32 else Fraction(float(shift))
    return np.array([dtype(float(Fraction(float(v)) * sc + sh)) for v in x], dtype=dtype)


def test_inputs_can_tell_a_contracted_multiply_add_from_the_two_roundings():
    # a condition on the inputs, checked on the CPU: in every (dtype, scale) case of the stage test some value of the 129-value layer
    # differs between NumPy's two roundings and the contracted form
    shift = -0.0123
    for code, scale in itertools.product((F64, F32, F16, BF16), SCALES):
        src = stored(layer_values(129, 7), code)
        for wide in ((False,) if code == F64 else (False, True)):
            flags = SC | SH | (SCW | O64 if wide or code == F64 else 0)
            ref = stage_ref(src, code, flags, scale, shift)
            x = np.asarray(src, dtype=np.float64) if code == F64 or wide else as_f32(src, code)
            fused = contracted(x.astype(ref.dtype), scale, shift, ref.dtype.type)
            if scale != 0.3 and (wide or code in (F16, BF16)):
                # a narrower value times 5000 or 37 (10 and 6 bits) is exact in the type the product is computed in -- 24 + 10 bits in
                # float64, 11 + 10 (float16) and 8 + 10 (bfloat16) in float32: there is no rounding a contraction could skip
                sc = ref.dtype.type(scale)
                assert all(Fraction(float(v)) * Fraction(float(sc)) == Fraction(float(ref.dtype.type(v) * sc)) for v in x), (code, scale, wide)
                continue
            assert (fused != ref).sum() >= 1, (code, scale, wide)


def test_stage_rows_against_numpy(eng):
    shift = -0.0123
    cases = []
    for code in (F64, F32, F16, BF16):
        for ci, (flags, size) in enumerate(itertools.product(stage_combos(code), SIZES)):
            cases.append((code, flags, size, SCALES[ci % 3], ci))
    total = sum(size for _c, _f, size, _s, _i in cases)
    src_a, dst_a = Arena(eng, 8 * total + 64 * len(cases)), Arena(eng, 8 * total + 64 * len(cases))
    rows, want = [], []
    for code, flags, size, scale, ci in cases:
        src = stored(layer_values(size, 1000 + ci), code)
        s_off = src_a.take(size, ES[code], ci % 2)
        d_es = 8 if flags & O64 else 4
        d_off = dst_a.take(size, d_es, (ci // 2) % 2)
        rows.append((src_a.put(s_off, src), dst_a.buf.ptr + d_off, size, scale, shift, code, flags))
        want.append((d_off, stage_ref(src, code, flags, scale, shift)))
    eng.stage_layers_dev(rows)
    for (code, flags, size, scale, _ci), (d_off, ref) in zip(cases, want):
        got = dst_a.get(d_off, ref.dtype, size)
        assert got.tobytes() == ref.tobytes(), (code, hex(flags), size, scale)
        # the bytes either side of the row are untouched
        assert (dst_a.get(d_off + ref.nbytes, np.uint8, 16) == 0xA5).all(), (code, hex(flags), size)


def test_stage_rows_without_a_scale_are_the_old_stage_pass(eng):
    # the same ciphertext from flashe_quantize_encrypt_tensors_dev's own stage pass (SHIFT / SHIFT_WIDE / LOOP_F64 rows) and from
    # flashe_stage_layers_dev followed by plain rows
    sizes, shift, alpha = [129, 8, 8193, 7], -0.0123, 0.25
    specs = [(F16, SH, _lib.TENSOR_SHIFT), (BF16, SH | SHW, _lib.TENSOR_SHIFT | _lib.TENSOR_SHIFT_WIDE), (F32, SH | O64, _lib.TENSOR_SHIFT | _lib.TENSOR_LOOP_F64),
             (F64, SH | O64, _lib.TENSOR_SHIFT)]
    n = sum(sizes)
    src_a, dst_a = Arena(eng, 8 * n + 256), Arena(eng, 8 * n + 256)
    old, stage, new, at = [], [], [], 0
    for li, ((code, sflags, oflags), size) in enumerate(zip(specs, sizes)):
        p = src_a.put(src_a.take(size, ES[code], li % 2), stored(layer_values(size, 50 + li), code))
        d = dst_a.buf.ptr + dst_a.take(size, 8 if sflags & O64 else 4, 0)
        old.append((at, p, alpha, shift, code, oflags))
        stage.append((p, d, size, 1.0, shift, code, sflags))
        new.append((at, d, alpha, 0.0, F64 if sflags & O64 else F32, 0))
        at += size
    du = eng.upload(np.random.Generator(np.random.PCG64(5)).random(n))
    cts = []
    for table in (old, new):
        if table is new:
            eng.stage_layers_dev(stage)
        ct = eng.alloc_vec(n)
        eng.quantize_encrypt_tensors_dev(3, 0, 1, n, 16, 0, n, table, 16, du, ct)
        cts.append(ct.download(np.uint64, 2 * n).tobytes())
    assert cts[0] == cts[1]


# ---------------------------------------------------------------- the finish pass against NumPy
def finish_ref(x, flags, s, shift, own, last64):
    """jzf_aggregator.py:902-907 on a float64 layer; returns (y2 as the statistics see it, y4)."""
    y = x
    if flags & DT:
        y = y / s
    if flags & FSH:
        y = y + shift
    y2 = y
    if flags & DO:
        y = y / own
    if flags & AL:
        y = last64 + y
    return y2, y


def test_inputs_can_tell_the_divisions_from_their_shortcuts():
    x = layer_values(129, 11)
    for total, own in DIVISORS:
        s = total / own
        assert (x / s != x * (1 / s)).sum() >= 1, (total, own)
        assert ((x / s) / own != x / (s * own)).sum() >= 1, (total, own)
        assert ((x / s) / own != x / float(total)).sum() >= 1, (total, own)
        assert ((x + 0.5) / own != (x + 0.5) * (1 / own)).sum() >= 1, (total, own)


@pytest.mark.parametrize("dst_code", [F64, F32, F16, BF16])
def test_finish_rows_against_numpy(eng, dst_code):
    shift, block = 0.0123, 8192
    cases = [(flags, size) for flags in range(16) for size in SIZES]
    n = sum(size for _f, size in cases)
    x = layer_values(n, 21)
    din = eng.upload(x)
    dst_a, last_a = Arena(eng, 8 * n + 64 * len(cases)), Arena(eng, 8 * n + 64 * len(cases))
    rows, want, at = [], [], 0
    for ci, (flags, size) in enumerate(cases):
        total, own = DIVISORS[ci % 2]
        s = total / own
        d_off = dst_a.take(size, ES[dst_code], ci % 2)
        last_code = (F64, F32, F16, BF16)[(ci // 2) % 4]
        in_place = bool(flags & AL) and ci % 5 == 0
        if in_place:
            last_code = dst_code
        last = stored(layer_values(size, 3000 + ci), last_code)
        last_ptr = 0
        if in_place:
            last_ptr = dst_a.put(d_off, last)
        elif flags & AL:
            last_ptr = last_a.put(last_a.take(size, ES[last_code], (ci // 3) % 2), last)
        last64 = last.astype(np.float64) if last_code == F64 else as_f32(last, last_code).astype(np.float64)
        y2, y4 = finish_ref(x[at:at + size], flags, s, shift, float(own), last64)
        rows.append((at, dst_a.buf.ptr + d_off, last_ptr, s, shift, float(own), dst_code, last_code, flags))
        want.append((d_off, stored(y4, dst_code), y2))
        at += size
    stats = eng.alloc(16 * len(rows))
    eng.finish_layers_dev(din, n, rows, block=np.getbufsize(), stats=stats)
    assert np.getbufsize() == block
    st = stats.download(np.float64, 2 * len(rows))
    for ci, ((flags, size), (d_off, ref, y2)) in enumerate(zip(cases, want)):
        got = dst_a.get(d_off, ref.dtype, size)
        assert got.tobytes() == ref.tobytes(), (dst_code, flags, size)
        mean, std = np.float64(st[2 * ci]) / size, np.sqrt(np.float64(st[2 * ci + 1]) / size)
        assert float(mean).hex() == float(np.mean(y2)).hex() and float(std).hex() == float(np.std(y2)).hex(), (dst_code, flags, size)


def test_finish_rows_without_a_new_flag_are_store_layers(eng):
    n = sum(SIZES)
    x = layer_values(n, 31)
    din = eng.upload(x)
    for shift_on in (False, True):
        outs = []
        for new in (False, True):
            a = Arena(eng, 8 * n + 64 * len(SIZES))
            rows, offs, at = [], [], 0
            for li, size in enumerate(SIZES):
                code = (F64, F32, F16, BF16)[li % 4]
                off = a.take(size, ES[code], li % 2)
                offs.append((off, code, size))
                if new:
                    rows.append((at, a.buf.ptr + off, 0, 1.0, 0.5, 1.0, code, 0, FSH if shift_on else 0))
                else:
                    rows.append((at, a.buf.ptr + off, 1.0, 0.5, code, _lib.TENSOR_SHIFT if shift_on else 0))
                at += size
            stats = eng.alloc(16 * len(rows))
            (eng.finish_layers_dev if new else eng.store_layers_dev)(din, n, rows, block=np.getbufsize(), stats=stats)
            outs.append(([a.get(off, NPDT[code], size).tobytes() for off, code, size in offs], stats.download(np.float64, 2 * len(rows)).tobytes()))
        assert outs[0] == outs[1]


# ---------------------------------------------------------------- refusals: FLASHE_EINVAL, nothing launched
def _stage_call(eng, rows):
    arr = (_lib.StageRow * max(len(rows), 1))()
    for i, (src, dst, size, scale, shift, dtype, flags) in enumerate(rows):
        arr[i].src, arr[i].dst, arr[i].size, arr[i].scale, arr[i].shift, arr[i].src_dtype, arr[i].flags = src, dst, size, scale, shift, dtype, flags
    return eng._lib.flashe_stage_layers_dev(eng._h, arr, len(rows))


def _finish_call(eng, din, n, rows, block=0, stats=None):
    arr = (_lib.FinishRow * max(len(rows), 1))()
    for i, r in enumerate(rows):
        (arr[i].start, arr[i].dst, arr[i].last, arr[i].div_total, arr[i].shift, arr[i].div_own, arr[i].dst_dtype, arr[i].last_dtype, arr[i].flags,
         arr[i].reserved) = r
    return eng._lib.flashe_finish_layers_dev(eng._h, din, n, arr, len(rows), block, stats)


def _refused_in_a_capture(call):
    """The call on an engine of its own between graph_begin and graph_end: refused, and the capture still ends."""
    e2 = Engine(KEY, 128)
    e2.graph_begin()
    try:
        rc = call(e2)
    finally:
        try:
            e2.graph_end()
        except Exception:
            pass
    return rc == EINVAL


def test_stage_refusals_launch_nothing(eng):
    n = 16
    src, dst = eng.upload(np.ones(n, np.float32)), eng.alloc(8 * n)
    eng.memset_dev(dst, 0xA5, 8 * n)
    good = [src.ptr, dst.ptr, n, 5000.0, -0.5, F32, SC | SH]
    assert _stage_call(eng, [tuple(good)]) == 0
    eng.memset_dev(dst, 0xA5, 8 * n)
    bad = [(0, None), (1, None), (0, src.ptr + 2), (1, dst.ptr + 2), (5, 7), (6, 32 | SC), (6, SCW), (6, SHW), (6, SC | SCW), (6, SC | SCW | SH | SHW | O64),
           (3, 0.0), (3, float("inf")), (3, float("nan")), (4, float("nan"))]
    for field, value in bad:
        row = list(good)
        row[field] = value
        assert _stage_call(eng, [tuple(row)]) == EINVAL, (field, value)
    f64 = eng.upload(np.ones(n))
    assert _stage_call(eng, [(f64.ptr, dst.ptr, n, 1.0, 0.0, F64, 0)]) == EINVAL                     # a float64 source without OUT_F64
    assert _stage_call(eng, [(f64.ptr, dst.ptr, n, 2.0, 0.0, F64, SC | SCW | O64)]) == EINVAL        # a WIDE flag on a float64 source
    assert _refused_in_a_capture(lambda e2: _stage_call(e2, [tuple(good)]))
    eng.sync()
    assert (dst.download(np.uint8, 8 * n) == 0xA5).all()


def test_finish_refusals_launch_nothing(eng):
    n = 16
    din, dst, last, stats = eng.upload(np.ones(n)), eng.alloc(8 * n + 64), eng.upload(np.ones(n + 8, np.float32)), eng.alloc(64)
    eng.memset_dev(dst, 0xA5, 8 * n + 64)
    eng.memset_dev(stats, 0xA5, 64)
    good = [[0, dst.ptr, last.ptr, 2.74, 0.5, 5000.0, F32, F32, DT | FSH | DO | AL, 0], [8, dst.ptr + 32, last.ptr + 32, 2.74, 0.5, 5000.0, F32, F32, DT | FSH | DO | AL, 0]]
    assert _finish_call(eng, din.ptr, n, [tuple(r) for r in good], 8192, stats.ptr) == 0
    eng.sync()
    eng.memset_dev(dst, 0xA5, 8 * n + 64)
    eng.memset_dev(stats, 0xA5, 64)
    bad = [(0, 1, None), (0, 1, dst.ptr + 2), (0, 2, None), (0, 2, last.ptr + 2), (0, 6, 9), (0, 7, 9), (0, 8, 16 | DT), (0, 9, 1), (0, 3, 0.0),
           (0, 3, float("inf")), (0, 3, float("nan")), (0, 5, 0.0), (0, 5, float("-inf")), (0, 4, float("nan")), (0, 0, 1), (1, 0, n + 1),
           (0, 2, dst.ptr + 8),             # last partially over its own dst
           (0, 2, dst.ptr + 32),            # last over another row's dst
           (1, 2, dst.ptr)]                 # the same the other way round
    for r, field, value in bad:
        rows = [list(x) for x in good]
        rows[r][field] = value
        assert _finish_call(eng, din.ptr, n, [tuple(x) for x in rows], 8192, stats.ptr) == EINVAL, (r, field, value)
    rows = [list(x) for x in good]
    rows[0][2], rows[0][7] = dst.ptr, F16                                                       # last == dst with another dtype
    assert _finish_call(eng, din.ptr, n, [tuple(x) for x in rows], 8192, stats.ptr) == EINVAL
    rows = [list(x) for x in good]
    rows[0][0], rows[1][0] = 8, 0                                                               # starts that descend (and rows[0].start != 0)
    assert _finish_call(eng, din.ptr, n, [tuple(x) for x in rows], 8192, stats.ptr) == EINVAL
    g = [tuple(x) for x in good]
    assert _finish_call(eng, None, n, g, 8192, stats.ptr) == EINVAL
    assert _finish_call(eng, din.ptr + 4, n, g, 8192, stats.ptr) == EINVAL
    assert _finish_call(eng, din.ptr, n, g, 8192, stats.ptr + 4) == EINVAL
    assert _finish_call(eng, din.ptr, n, g, 0, stats.ptr) == EINVAL
    assert _finish_call(eng, din.ptr, n, g, 16385, stats.ptr) == EINVAL
    assert _finish_call(eng, din.ptr, n, [], 8192, stats.ptr) == EINVAL
    assert _refused_in_a_capture(lambda e2: _finish_call(e2, din.ptr, n, g, 8192, stats.ptr))
    eng.sync()
    assert (dst.download(np.uint8, 8 * n + 64) == 0xA5).all() and (stats.download(np.uint8, 64) == 0xA5).all()
    # in place with equal dtypes is fine
    rows = [list(x) for x in good]
    rows[0][2], rows[1][2] = dst.ptr, dst.ptr + 32
    assert _finish_call(eng, din.ptr, n, [tuple(x) for x in rows], 8192, stats.ptr) == 0
    eng.sync()


# ---------------------------------------------------------------- through the classes, with tensors on the device
class _W:
    def __init__(self, layers):
        self.walking_order = sorted(layers)
        self._weights = dict(layers)


class _Cai:
    """A framework-free device tensor: __cuda_array_interface__ v3 over an engine buffer."""
    TYPESTR = {F32: "<f4", F64: "<f8", F16: "<f2"}

    def __init__(self, buf, shape, code):
        self.buf, self.shape, self.code = buf, tuple(shape), code
        self.__cuda_array_interface__ = {"shape": self.shape, "typestr": self.TYPESTR[code], "data": (buf.ptr, False), "version": 3, "strides": None,
                                         "stream": None}


class TorchTensors:
    """torch tensors on the device, in the four dtypes."""
    half = BF16

    def __init__(self, torch):
        self.torch = torch
        self.dt = {F32: torch.float32, F64: torch.float64, F16: torch.float16, BF16: torch.bfloat16}

    def tensor(self, carrier, code, shape):
        t = self.torch
        x = t.from_numpy(np.ascontiguousarray(carrier).view(np.int16)).view(t.bfloat16) if code == BF16 else t.from_numpy(np.ascontiguousarray(carrier))
        return x.reshape(shape).cuda()

    def empty(self, shape, code):
        return self.torch.empty(shape, dtype=self.dt[code], device="cuda")

    def read(self, x, code):
        x = x.cpu().reshape(-1)
        return x.view(self.torch.int16).numpy().view(np.uint16) if code == BF16 else x.numpy()


class CaiTensors:
    """The same without a framework (float64 / float32 / float16: the interface has no bfloat16), for a machine whose torch sees no device."""
    half = F16

    def __init__(self):
        self.eng = Engine(KEY, 64)

    def tensor(self, carrier, code, shape):
        carrier = np.ascontiguousarray(carrier)
        return _Cai(self.eng.alloc(max(carrier.nbytes, 16)).upload(carrier), shape, code)

    def empty(self, shape, code):
        return _Cai(self.eng.alloc(max(int(np.prod(shape)) * ES[code], 16)), shape, code)

    def read(self, x, code):
        return x.buf.download(NPDT[code], int(np.prod(x.shape)))


@pytest.fixture(scope="module", params=["torch", "cai"])
def dev(request):
    """torch tensors where torch sees the device (skipped otherwise, as test_gpu_tensor_interop.py does), and the framework-free producer:
    every case runs on a machine without a usable torch too."""
    if request.param == "cai":
        return CaiTensors()
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible to torch")
    return TorchTensors(torch)


def _args(b, batch=False, element_bits=16, precompute=None):
    return {"quantize": {"int_bits": b, "batch": batch, "element_bits": element_bits, "padding": True, "secure": True},
            "precompute": {"enable": precompute is not None, "num_params": precompute}}


SHAPES = {"a": (129,), "b": (3, 43), "c": (8193,)}


def _model(dev, seed, shapes=SHAPES, codes=None):
    """({name: device tensor}, {name: its host copy as the host path takes it: 16-bit layers upcast to float32 exactly})."""
    codes = codes or {"a": F32, "b": F64, "c": dev.half}
    tensors, host = {}, {}
    for i, (k, shape) in enumerate(shapes.items()):
        carrier = stored(layer_values(int(np.prod(shape)), 100 * seed + i), codes[k])
        tensors[k] = dev.tensor(carrier, codes[k], shape)
        host[k] = (carrier if codes[k] in (F32, F64) else as_f32(carrier, codes[k])).reshape(shape)
    return tensors, host


def _client(b, idx=0, C=3, degree=1.0, shapes=SHAPES, **kw):
    """A keyed client whose quantiser holds the statistics a previous round's unnormalize leaves for a model scaled by `degree`
    (np.float64 values: the means shift in float64, the alphas are np.float64)."""
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheClient
    cm.N_JOBS = 16
    cl = FlasheClient(_args(b, **kw))
    cl.create_cipher(idx, C, KEY)
    cl.set_iter_index(5)
    q = cl.quantizer
    q.layer_size_list = [int(np.prod(s)) for s in shapes.values()]
    q.past_layer_mean_list = [np.float64(0.0123 * float(degree) * (i + 1)) for i in range(len(shapes))]
    q.past_layer_std_list = [np.float64(0.05 * float(degree)) for _ in shapes]
    return cl


def _stats(cl):
    q = cl.quantizer
    return list(q.past_layer_mean_list), list(q.past_layer_std_list)


def _set_stats(cl, snap):
    cl.quantizer.past_layer_mean_list, cl.quantizer.past_layer_std_list = list(snap[0]), list(snap[1])


def _hex(xs):
    return [float(x).hex() for x in xs]


def _host_sequence(cl, agg, total, degree, last_host, unnormalize=True):
    """jzf_aggregator.py:887-907 written out: the existing decrypt_unquantize, `/ (total / degree)`, the existing unnormalize, `/ degree`,
    `last + w`, on host arrays."""
    w = cl.decrypt_unquantize(_W({next(iter(cl.shape_dict)): agg}))
    for k in w.walking_order:
        w._weights[k] = w._weights[k] / (total / degree)
    if unnormalize:
        w = cl.unnormalize(w)
    for k in w.walking_order:
        w._weights[k] = w._weights[k] / degree
        if last_host is not None:
            w._weights[k] = last_host[k] + w._weights[k]
    return w


def _same(dev, tensor, code, y64):
    """The device tensor holds the float64 host result as its dtype stores it (float64 -> float32 -> 16 bits), byte for byte."""
    return dev.read(tensor, code).tobytes() == stored(np.asarray(y64, dtype=np.float64).reshape(-1), code).tobytes()


@pytest.mark.parametrize("b", [128, 20])
@pytest.mark.parametrize("degree", [5000.0, np.float64(37.0)], ids=["float", "np.float64"])
def test_client_round_with_tensors(dev, b, degree):
    total = 13700 if float(degree) == 5000.0 else 111
    tensors, host = _model(dev, 3)
    before = {k: dev.read(v, c).tobytes() for (k, v), c in zip(tensors.items(), (F32, F64, dev.half))}
    ref, got = _client(b, C=1, degree=degree), _client(b, C=1, degree=degree)       # (a federation of one: its upload is the aggregate)
    np.random.seed(9)
    want = ref.quantize_encrypt(_W({k: v * degree for k, v in host.items()}), normalize=True)
    np.random.seed(9)
    up = got.quantize_encrypt(_W(dict(tensors)), normalize=True, degree=degree)
    agg = up._weights[up.walking_order[0]].to_host()
    assert agg.tobytes() == want._weights[want.walking_order[0]].to_host().tobytes()
    assert _hex(got.quantizer.alpha_list) == _hex(ref.quantizer.alpha_list) and got.degree is degree
    assert before == {k: dev.read(v, c).tobytes() for (k, v), c in zip(tensors.items(), (F32, F64, dev.half))}     # the caller's tensors are never written
    snap = _stats(ref)
    for out_code, in_place in itertools.product((F32, dev.half), (False, True)):
        for cl in (ref, got):
            _set_stats(cl, snap)
            cl.set_idx_list([0])
        last_c = {k: stored(layer_values(int(np.prod(s)), 70 + i), out_code) for i, (k, s) in enumerate(SHAPES.items())}
        last_t = {k: dev.tensor(last_c[k], out_code, SHAPES[k]) for k in SHAPES}
        last_h = {k: (last_c[k] if out_code == F32 else as_f32(last_c[k], out_code)).astype(np.float64).reshape(SHAPES[k]) for k in SHAPES}
        w = _host_sequence(ref, agg.copy(), total, degree, last_h)
        out = last_t if in_place else {k: dev.empty(SHAPES[k], out_code) for k in SHAPES}
        res = got.decrypt_unquantize(_W({"a": agg.copy()}), out=out, unnormalize=True, total_degree=total, last_round=last_t)
        for k in SHAPES:
            assert res._weights[k] is out[k]
            assert _same(dev, out[k], out_code, w._weights[k]), (b, k, out_code, in_place)
            assert in_place or dev.read(last_t[k], out_code).tobytes() == last_c[k].tobytes()
        assert _hex(got.quantizer.past_layer_mean_list) == _hex(ref.quantizer.past_layer_mean_list)
        assert _hex(got.quantizer.past_layer_std_list) == _hex(ref.quantizer.past_layer_std_list)
        assert _hex(got.quantizer.past_layer_mean_list) != _hex(snap[0])


def test_batched_and_prepared_rounds_with_tensors(dev):
    degree, total = 5000.0, 13700
    tensors, host = _model(dev, 4)
    n = sum(int(np.prod(s)) for s in SHAPES.values())
    for kw in (dict(batch=True, element_bits=16), dict(precompute=n)):
        b = 120 if kw.get("batch") else 128
        ref, got = _client(b, C=1, degree=degree, **kw), _client(b, C=1, degree=degree, **kw)
        np.random.seed(2)
        want = ref.quantize_encrypt(_W({k: v * degree for k, v in host.items()}), normalize=True)
        np.random.seed(2)
        up = got.quantize_encrypt(_W(dict(tensors)), normalize=True, degree=degree)
        agg = up._weights[up.walking_order[0]].to_host()
        assert agg.tobytes() == want._weights[want.walking_order[0]].to_host().tobytes(), kw
        for cl in (ref, got):
            cl.prepare_decrypt()
            cl.set_idx_list([0])
        w = _host_sequence(ref, agg.copy(), total, degree, None)
        out = {k: dev.empty(SHAPES[k], F32) for k in SHAPES}
        got.decrypt_unquantize(_W({"a": agg.copy()}), out=out, unnormalize=True, total_degree=total)
        for k in SHAPES:
            assert _same(dev, out[k], F32, w._weights[k]), (kw, k)
        assert _hex(got.quantizer.past_layer_mean_list) == _hex(ref.quantizer.past_layer_mean_list)
        assert _hex(got.quantizer.past_layer_std_list) == _hex(ref.quantizer.past_layer_std_list)


def test_sparse_back_end_with_location_masks(dev):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheSparseCohort
    cm.N_JOBS = 16
    degree, total, C = 37.0, 111, 3
    shapes = {"a": (1290,), "b": (30, 43)}
    names = list(shapes)
    last_c = {k: stored(layer_values(int(np.prod(s)), 90 + i), F32) for i, (k, s) in enumerate(shapes.items())}
    results = []
    for on_device in (False, True):
        co = FlasheSparseCohort(dict(_args(20), mask="dynamic"), first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, sparsity=0.1)
        g = np.random.Generator(np.random.PCG64(8))
        models = [{k: (g.standard_normal(s) * 0.05).astype(np.float32) for k, s in shapes.items()} for _ in range(C)]
        co.sparsify(models, names)
        co.set_iter_index(1)
        assert co.dynamic_masking() == "single"
        np.random.seed(4)
        co.quantize_encrypt(normalize=True)
        if on_device:
            out = {k: dev.empty(s, F32) for k, s in shapes.items()}
            last_t = {k: dev.tensor(last_c[k], F32, shapes[k]) for k in names}
            co.decrypt_unquantize(out=out, unnormalize=True, degree=degree, total_degree=total, last_round=last_t)
            vals = {k: dev.read(out[k], F32).tobytes() for k in names}
        else:
            w = co.decrypt_unquantize()
            for k in w.walking_order:
                w._weights[k] = w._weights[k] / (total / degree)
            w = co.lead.unnormalize(w)
            vals = {k: stored((last_c[k].astype(np.float64) + (w._weights[k] / degree).reshape(-1)), F32).tobytes() for k in names}
        q = co.lead.quantizer
        results.append((vals, _hex(q.past_layer_mean_list), _hex(q.past_layer_std_list)))
    assert results[0] == results[1]


def _cohort(n_local, b=128):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheCohort
    cm.N_JOBS = 16
    co = FlasheCohort(_args(b), first_idx=0, n_local=n_local, num_clients=n_local, prp_seed=KEY)
    co.set_iter_index(5)
    return co


@pytest.mark.parametrize("form", ["cohort-chain", "staged-chain"])
def test_cohort_round_with_tensors(dev, form):
    from flashe_amd.block import cohort_admission_length
    C, degrees = 3, [5000.0, 3700, np.float32(5000.0)]
    big = cohort_admission_length(_cohort(C).cipher.engine.cu_count) + 3 if form == "cohort-chain" else 300
    shapes = {"a": (129,), "b": (big,), "c": (3, 43)}
    codes = {"a": F32, "b": F32, "c": dev.half}
    models = [_model(dev, 12 + c, shapes, codes) for c in range(C)]
    for present in (None, [0, 2]):
        pos = list(range(C)) if present is None else present
        degs = [degrees[p] for p in pos]
        co = _cohort(C)
        ref = _client(128, C=C, shapes=shapes, degree=5000.0)
        _set_stats(co.lead, _stats(ref))
        co.quantizer.layer_size_list = list(ref.quantizer.layer_size_list)
        np.random.seed(6)
        up = co.quantize_encrypt([_W(dict(models[p][0])) for p in pos], normalize=True, present=present, degrees=degs)
        assert up.path == form, (up.path, present)
        # the host sequence, client by client
        np.random.seed(6)
        snap = _stats(ref)
        for ci, p in enumerate(pos):
            ref.cipher.idx = p
            want = ref.quantize_encrypt(_W({k: v * degs[ci] for k, v in models[p][1].items()}), normalize=True)
            assert up.ciphertexts[ci].to_host().tobytes() == want._weights[want.walking_order[0]].to_host().tobytes(), (form, present, ci)
        assert _stats(ref) == snap
        # the cohort's own-sum decrypt: degree = the first present client's, total_degree = the left-to-right sum of the present ones
        total = functools.reduce(operator.add, degs)
        ref.cipher.idx = 0
        ref.set_idx_list(pos)
        w = _host_sequence(ref, up.partial_sum.to_host(), total, degs[0], None)
        out = {k: dev.empty(s, F32) for k, s in shapes.items()}
        co.decrypt_unquantize(out=out, unnormalize=True)
        for k in shapes:
            assert _same(dev, out[k], F32, w._weights[k]), (form, present, k)
        assert _hex(co.quantizer.past_layer_mean_list) == _hex(ref.quantizer.past_layer_mean_list)
        assert _hex(co.quantizer.past_layer_std_list) == _hex(ref.quantizer.past_layer_std_list)
