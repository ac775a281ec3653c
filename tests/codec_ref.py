"""An independent reference of the quantise / batch codec, and the planes of edge inputs its tests feed (a plain helper, no conftest).

The reference is the codec's published arithmetic written down once more, in NumPy for the way in and on Python ints for the way back --
deliberately NOT the oracle (oracle/flashe_oracle.c), whose codec is a line-for-line twin of the device code:

    quantise    v = clip(x, -alpha, alpha) + alpha;  v = v * (2^bits - 1) / (2 * alpha);  floor(v + u).astype(int)
                in the array's own dtype with alpha a Python float (a weak scalar); u is float64, so the last step is float64
    unquantise  a = alpha * C;  value * (2 * a) / ((2^bits - 1) * C) - a        on Python ints: int -> float and float / int are
                correctly rounded, whatever the width of the int
    batch       t = t * 2^field_bits + v, first value most significant, zero padded to int_bits // field_bits values per element
    normalise   array += scalar, in the loop dtype NumPy itself picks

Two rules keep a case out of the plane, both because the reference itself is platform-defined there (conditions, not measurements):
  * no NaN input: floor(nan).astype(int) is whatever the platform's cast gives;
  * no (dtype, alpha, bits) whose largest scaled image 2 * alpha * (2^bits - 1) overflows the dtype: the cast of +-inf to int is
    platform-defined too (x86 and gfx950 differ, and neither is "the reference").
Everything else stays: +-0, +-alpha and their neighbours, +-inf, subnormals, the dtype's extremes, values whose scaled image is an
integer or one ulp off it, every width from 1 to 62 bits.  A case the rules drop is dropped when the plane is built, and the plane says how
many it kept, so a test can hold a floor against an over-eager filter.

The last section builds whole cohorts for the fused cohort launches (cohort_model and what hangs off it): C clients' models of rows in
every storage format, filled by layer_fill, with the plaintexts the reference quantises them to -- q == 2^bits and 2^bits + 1 kept as they
are -- and the batched elements, in which such a q carries out of a field that is exactly element_bits wide.
"""
from fractions import Fraction

import numpy as np

ALPHAS = (8.17121, 0.1, 1.0, 3e-3, 1e-30, 1e30)
WIDTHS = (1, 2, 8, 16, 23, 24, 25, 31, 32, 33, 52, 53, 54, 62)          # the plain kernels
FUSED_WIDTHS = (1, 16, 24, 32, 33, 53, 62)                              # the fused ones (those <= int_bits)
ONE_BELOW = float(np.nextafter(1.0, 0.0))                               # the largest draw np.random.random can make: 1 - 2^-53
DRAWS = ("zero", "one_below", "half", "random")
PAIRS = ((16, 10), (32, 10), (32, 1000), (53, 3), (62, 4), (62, 5), (62, 10), (58, 100), (40, 1 << 24), (33, (1 << 31) - 1))
WRAPPING_PAIRS = ((62, 5), (62, 10), (58, 100))                         # (2^bits - 1) * C >= 2^64


# ---------------------------------------------------------------------------------------------------------------- the reference
def loop_dtype(arr_dtype, scalar):
    """The dtype NumPy computes `array <op> scalar` in, asked of the running NumPy (a Python float is weak, an np.float64 is not)."""
    return (np.zeros(1, dtype=arr_dtype) + scalar).dtype


def upcast16(x):
    """A 16-bit source as the float32 array the codec computes on (exact).  x: np.float16 array, or a torch CPU tensor (bfloat16)."""
    if isinstance(x, np.ndarray):
        assert x.dtype == np.float16
        return x.astype(np.float32)
    import torch
    return x.detach().cpu().to(torch.float32).numpy()


def ref_scaled(x, alpha, bits):
    """The scaled image before the stochastic rounding, in x's dtype."""
    alpha = float(alpha)
    x = np.asarray(x)
    assert x.dtype in (np.float32, np.float64) and not np.isnan(x).any()
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.clip(x, -alpha, alpha) + alpha
        v = v * ((1 << bits) - 1) / (2 * alpha)
    assert v.dtype == x.dtype
    return v


def ref_quantize(x, alpha, bits, u):
    u = np.asarray(u, dtype=np.float64)
    v = ref_scaled(x, alpha, bits)
    q = np.floor(v + u).astype(np.int64)
    # every kept case lands in [0, 2^bits], the upper end included (float32 rounds 2^bits - 1 up to 2^bits from 25 bits on).  One step
    # beyond is reachable in exactly one way, and it is the reference's own float64 addition: an image of exactly 2^bits plus a draw so
    # close to 1 that the sum rounds to the integer 2^bits + 1 (1 - 2^-53 does that from 2^bits >= 2 on)
    top = 1 << bits
    assert q.size == 0 or (0 <= float(v.min()) and float(v.max()) <= top), (alpha, bits, float(v.min()), float(v.max()))
    assert ((q >= 0) & ((q <= top) | ((v == top) & (v + u == top + 1)))).all(), (alpha, bits, int(q.min()), int(q.max()))
    return q


def ref_unquantize(ints, alpha, bits, C):
    """ints: anything that iterates as Python ints.  Returns float64."""
    a = float(alpha) * C
    den = ((1 << bits) - 1) * C
    out = np.empty(len(ints), dtype=np.float64)
    for j, v in enumerate(ints):
        out[j] = int(v) * (2 * a) / den - a
    return out


def ref_batch(vals, int_bits, field_bits):
    bs = int_bits // field_bits
    vals = [int(v) for v in vals]
    out = []
    for b in range(0, len(vals), bs):
        t = 0
        for i in range(bs):
            t = t * 2 ** field_bits + (vals[b + i] if b + i < len(vals) else 0)
        out.append(t)
    return out


def ref_unbatch(items, int_bits, field_bits):
    bs = int_bits // field_bits
    out = []
    for t in items:
        t = int(t)
        vals = []
        for _ in range(bs):
            vals.append(t % 2 ** field_bits)
            t //= 2 ** field_bits
        out.extend(reversed(vals))
    return out


def ref_shift(x, shift):
    """normalise / unnormalise: `array += scalar` (loop in NumPy's own choice of dtype, result cast back)."""
    y = np.array(x, copy=True)
    with np.errstate(over="ignore"):
        y += shift
    return y


def to_limbs(ints, limbs):
    out = np.zeros((len(ints), limbs), dtype=np.uint64)
    m64 = (1 << 64) - 1
    for j, v in enumerate(ints):
        v = int(v)
        assert 0 <= v < 1 << (64 * limbs)
        out[j, 0] = v & m64
        if limbs == 2:
            out[j, 1] = v >> 64
    return out


def from_limbs(arr):
    arr = np.asarray(arr, dtype=np.uint64)
    if arr.ndim == 1:
        return [int(v) for v in arr]
    return [sum(int(w) << (64 * i) for i, w in enumerate(row)) for row in arr]


# ---------------------------------------------------------------------------------------------------------------- the edge plane
def overflows(dtype, alpha, bits):
    """Rule 2: the largest scaled image, 2 * alpha * (2^bits - 1), is not finite in the dtype."""
    dt = np.dtype(dtype).type
    with np.errstate(over="ignore"):
        top = dt(2 * float(alpha)) * dt((1 << bits) - 1)
        return not (np.isfinite(top) and np.isfinite(dt(alpha)))


def quantize_cases(dtype, alphas=ALPHAS, widths=WIDTHS):
    """The (alpha, bits) cases of `dtype` the two rules keep, and how many they dropped."""
    kept = [(a, w) for a in alphas for w in widths if not overflows(dtype, a, w)]
    return kept, len(alphas) * len(widths) - len(kept)


def _integer_images(dtype, alpha, widths):
    """Values whose scaled image at some width is an exact integer k or one ulp either side of it: the map is inverted in exact
    rationals, the few floats around the pre-image are tried, and only those the reference maps where intended are kept."""
    dt = np.dtype(dtype)
    A = Fraction(float(alpha))
    out = []
    for w in widths:
        if overflows(dt, alpha, w):
            continue
        S = (1 << w) - 1
        for k in sorted(k for k in {0, 1, 2, 3, S // 3, S // 2, (S + 1) // 2, S - 2, S - 1, S} if 0 <= k <= S):
            kf = dt.type(k)
            if int(kf) != k:                                            # k itself is not a value of the dtype
                continue
            targets = {float(kf), float(np.nextafter(kf, dt.type(np.inf))), float(np.nextafter(kf, dt.type(-np.inf)))}
            x0 = dt.type(float(Fraction(k) * 2 * A / S - A))
            cand = [x0]
            lo = hi = x0
            for _ in range(4):
                lo, hi = np.nextafter(lo, dt.type(-np.inf)), np.nextafter(hi, dt.type(np.inf))
                cand += [lo, hi]
            cand = np.array(cand, dtype=dt)
            img = ref_scaled(cand, alpha, w)
            out.extend(cand[[float(v) in targets for v in img]].tolist())
    return np.array(out, dtype=dt)


def edge_plane(dtype, alpha, n_fill=20000, seed=0, widths=WIDTHS, storage=None):
    """The x vector of the edge plane for `dtype` (np.float32 / np.float64) and `alpha`.  storage="float16" / "bfloat16" returns the
    plane of a 16-bit source instead: float32 values that are exactly representable in that format, with the format's own extremes."""
    dt = np.dtype(dtype)
    f, a = dt.type, dt.type(alpha)
    inf, fi = f(np.inf), np.finfo(dt)
    edges = [f(0.0), f(-0.0), a, -a, np.nextafter(a, inf), np.nextafter(a, f(0)), np.nextafter(-a, -inf), np.nextafter(-a, f(0)),
             inf, -inf, fi.tiny, -fi.tiny, fi.smallest_subnormal, -fi.smallest_subnormal, np.nextafter(fi.tiny, f(0)), fi.max, -fi.max]
    rng = np.random.RandomState(seed)
    with np.errstate(over="ignore"):
        gauss = (rng.standard_normal(n_fill) * float(alpha) * 0.4).astype(dt)
        line = np.linspace(-float(alpha), float(alpha), 4097).astype(dt)
    x = np.concatenate([np.array(edges, dtype=dt), _integer_images(dt, alpha, widths), line, gauss])
    if storage is not None:
        assert dt == np.float32
        x = _through16(x, storage)
    assert not np.isnan(x).any()
    return x


def _through16(x, storage):
    """x rounded to the 16-bit format (so every value is one the format holds), plus the format's extremes; returned as float32."""
    if storage == "float16":
        with np.errstate(over="ignore"):
            h = x.astype(np.float16)
        fi = np.finfo(np.float16)
        extra = np.array([65504.0, -65504.0, fi.smallest_subnormal, -fi.smallest_subnormal, np.nextafter(fi.tiny, np.float16(0)),
                          -np.nextafter(fi.tiny, np.float16(0))], dtype=np.float16)
        return np.concatenate([extra, h]).astype(np.float32)
    assert storage == "bfloat16"
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16)
    extra = torch.tensor([3.3895313892515355e38, -3.3895313892515355e38, 9.183549615799121e-41, -9.183549615799121e-41],
                         dtype=torch.float32).to(torch.bfloat16)          # the largest finite and the smallest subnormal bfloat16
    return torch.cat([extra, t]).to(torch.float32).numpy()


def draws(kind, n, seed=0):
    if kind == "zero":
        return np.zeros(n)
    if kind == "one_below":
        return np.full(n, ONE_BELOW)
    if kind == "half":
        return np.full(n, 0.5)
    assert kind == "random"
    return np.random.RandomState(seed + 77).random_sample(n)


def mixed_draws(n, seed=0):
    """One vector that holds all four kinds: element j takes kind j % 4 (0.0, 1 - 2^-53, 0.5, random)."""
    u = np.random.RandomState(seed + 78).random_sample(n)
    u[0::4] = 0.0
    u[1::4] = ONE_BELOW
    u[2::4] = 0.5
    return u


def crossed_plane(dtype, alpha, n_fill=3000, seed=0, storage=None):
    """(x, u) for a path that takes one launch per case: the plane four times over, each copy under one kind of draw."""
    x = edge_plane(dtype, alpha, n_fill, seed, storage=storage)
    return np.tile(x, 4), np.concatenate([draws(kind, len(x), seed) for kind in DRAWS])


def layer_fill(dtype, alpha, size, seed=0, storage=None):
    """`size` values for one layer of a model: the plane repeated (an odd period, so that under mixed_draws every value meets every
    kind of draw), with an edge value as the layer's first and last element."""
    x = edge_plane(dtype, alpha, 1500, seed, storage=storage)
    if len(x) % 2 == 0:
        x = x[:-1]
    x = np.resize(x, size)
    if size:
        x[0], x[-1] = np.nextafter(x.dtype.type(alpha), x.dtype.type(np.inf)), -x.dtype.type(alpha)
        if storage is not None:
            x[0], x[-1] = np.inf, -np.inf
    return x


def check_properties(x, alpha, bits, q, u):
    """What the plane implies, whatever produced q (names the element on failure)."""
    x, q, u = np.asarray(x), np.asarray(q).astype(np.int64), np.asarray(u)
    a = x.dtype.type(alpha)
    top = ref_quantize(np.array([a], dtype=x.dtype), alpha, bits, [0.0])[0]
    # (2 * alpha) * S / (2 * alpha) takes three roundings (alpha + alpha is exact), each within eps / 2 relative: within 1.5 * eps * S of
    # S = 2^bits - 1, so S - 1, S or S + 1 while S * eps < 1/2 and proportionally further above
    S = (1 << bits) - 1
    assert abs(int(top) - S) <= max(1, int(np.ceil(2 * float(np.finfo(x.dtype).eps) * S))), (alpha, bits, top)
    hi = (x >= a) & (u == 0.0)
    assert (q[hi] == top).all(), ("x >= alpha, draw 0", alpha, bits, x[hi][q[hi] != top][:4])
    lo = (x <= -a) & ((u == 0.0) | (u == ONE_BELOW))
    assert (q[lo] == 0).all(), ("x <= -alpha", alpha, bits, x[lo][q[lo] != 0][:4])
    zero = x == 0
    for draw in np.unique(u[zero]):
        assert len(set(q[zero & (u == draw)].tolist())) == 1, ("+-0 quantise alike", alpha, bits, draw)


# ---------------------------------------------------------------------------------------------------------------- the sum plane
def sum_plane(bits, C, int_bits=128, n_random=3000, seed=0):
    """Aggregates for the way back, as Python ints below 2^int_bits: the ends of the range the codec produces (top = (2^bits - 1) * C),
    and the places where int -> float64 has to round half to even (2^53, 2^64 + 2^11, 2^117 + 2^64, 2^127 + 2^74)."""
    top = ((1 << bits) - 1) * C
    pts = [0, 1, top, top - 1, top // 2]
    pts += [(1 << 53) + d for d in (0, 1, 2, 3)]
    pts += [(1 << 64) + d for d in (-1, 0, 1, 1 << 11, (1 << 11) + 1, 3 << 11)]
    pts += [(1 << 117) + (1 << 64) + d for d in (-1, 0, 1)]
    pts += [(1 << 127) + d for d in (1 << 74, (1 << 74) + 1, 3 << 74)]
    pts += [(1 << 128) - 1]
    rng = np.random.RandomState(seed + bits)
    for _ in range(n_random):
        nb = int(rng.randint(1, int_bits + 1))
        v = int.from_bytes(rng.bytes(16), "little") >> (128 - nb)
        pts.append(v | (1 << (nb - 1)))
    return [p for p in pts if 0 <= p < (1 << int_bits)]


# ---------------------------------------------------------------------------------------------------------------- cohort models
F32, F64, F16, BF16 = 0, 1, 2, 3                                        # flashe_tensor_layer dtype codes (include/flashe.h)
SHIFT, SHIFT_WIDE, LOOP_F64 = 1, 2, 4                                   # and flags
_STORAGE = {"float32": F32, "float64": F64, "float16": F16, "bfloat16": BF16}


def bits16(x32, storage):
    """The 16-bit patterns of float32 values the format holds exactly."""
    if storage == "float16":
        return x32.astype(np.float16).view(np.uint16)
    assert storage == "bfloat16"
    return (np.ascontiguousarray(x32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


class CohortModel:
    """What cohort_model returns: spec, C, sizes, starts, n; rows = the shared table (start, None, alpha, shift, compute dtype code, flags);
    dts[l] = layer l's storage dtype code; storage[c][l] = what client c holds in memory (float arrays, uint16 patterns for the 16-bit
    formats); ref[c][l] = the compute-type array the codec quantises (upcast, shifted, widened); u = mixed_draws(C * n), client-major."""


def cohort_model(spec, C, seed=0):
    """A cohort's model from rows of (storage, alpha, shift, wide, loop64, size): every client's every row is layer_fill's (an edge value
    either side of every row boundary), the draws are mixed_draws."""
    m = CohortModel()
    m.spec, m.C = list(spec), C
    m.sizes = [s[5] for s in m.spec]
    m.starts = [int(v) for v in np.concatenate([[0], np.cumsum(m.sizes)[:-1]])]
    m.n = int(sum(m.sizes))
    m.rows, m.dts = [], []
    for (storage, alpha, shift, wide, loop64, _size), start in zip(m.spec, m.starts):
        flags = (SHIFT if shift is not None else 0) | (SHIFT_WIDE if shift is not None and wide else 0) | (LOOP_F64 if loop64 else 0)
        m.rows.append((start, None, alpha, 0.0 if shift is None else shift, F64 if storage == "float64" else F32, flags))
        m.dts.append(_STORAGE[storage])
    m.storage, m.ref = [], []
    for c in range(C):
        held, ref = [], []
        for li, (storage, alpha, shift, wide, loop64, size) in enumerate(m.spec):
            half = storage in ("float16", "bfloat16")
            x = layer_fill(np.float64 if storage == "float64" else np.float32, alpha, size, seed + 10 * c + li, storage=storage if half else None)
            held.append(bits16(x, storage) if half else x.copy())
            if shift is not None:
                x = ref_shift(x, np.float64(shift) if wide else float(shift))
            if loop64:
                x = x.astype(np.float64)
            ref.append(x)
        m.storage.append(held)
        m.ref.append(ref)
    m.u = mixed_draws(C * m.n, seed)
    return m


def _cohort_rows_q(model, bits, c):
    u = model.u[c * model.n:(c + 1) * model.n]
    return [ref_quantize(x, row[2], bits, u[at:at + len(x)]) for x, row, at in zip(model.ref[c], model.rows, model.starts)]


def cohort_plaintexts(model, bits):
    """Per client the concatenated ref_quantize of its rows as int64 (bits <= 62: Python-int safe); 2^bits and 2^bits + 1 are kept."""
    return [np.concatenate(_cohort_rows_q(model, bits, c) + [np.zeros(0, np.int64)]) for c in range(model.C)]


def cohort_batched(model, bits, int_bits, field_bits):
    """Per client the batched plaintext as Python ints: ref_batch of every row on its own (each padded to whole elements), reduced
    mod 2^int_bits as the cipher reduces it."""
    return [[t % (1 << int_bits) for q in _cohort_rows_q(model, bits, c) for t in ref_batch(q, int_bits, field_bits)] for c in range(model.C)]


def cohort_field_overflows(model, bits, int_bits, field_bits):
    """Where a quantised value does not fit its field: (client, row, element of the row, slot, the row's element count, the row's size)
    for every q >= 2^field_bits.  Slot 0 is the most significant field; an overflow there carries out of bit bs * field_bits."""
    bs, out = int_bits // field_bits, []
    for c in range(model.C):
        for li, q in enumerate(_cohort_rows_q(model, bits, c)):
            for j in np.flatnonzero(q >= (1 << field_bits)):
                out.append((c, li, int(j) // bs, int(j) % bs, -(-len(q) // bs), len(q)))
    return out


def check_cohort_case(model, bits):
    """The conditions a cohort case meets on the reference alone: no row under overflows() (asserted, not filtered), every client holds a
    q == 2^bits, and a case with a float32 compute row at bits >= 25 holds a q == 2^bits + 1 (float32 rounds the image 2^bits - 1 up to
    2^bits there, and the float64 sum 2^bits + (1 - 2^-53) rounds to 2^bits + 1 -- while that integer is a float64 at all, bits <= 52;
    beyond, the sum is 2^bits itself)."""
    for x, row in zip(model.ref[0], model.rows):
        assert not overflows(x.dtype, row[2], bits), (x.dtype, row[2], bits)
    pts = cohort_plaintexts(model, bits)
    for c, q in enumerate(pts):
        assert (q == 1 << bits).any(), ("no q == 2^bits", c, bits)
    if 25 <= bits <= 52 and any(x.dtype == np.float32 and len(x) for x in model.ref[0]):
        assert any((q == (1 << bits) + 1).any() for q in pts), ("no q == 2^bits + 1", bits)
    return pts
