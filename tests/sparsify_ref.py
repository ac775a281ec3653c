"""An independent reference of the top-k sparsifier, and the edge inputs its tests feed (a plain helper: NumPy only, no GPU, no ctypes).

The reference is Client.sparsify for one layer (jzf_aggregator.py:578-623) written down once more:

    rank      np.argsort(|layer| as float64, kind="stable"), the last k, ascending: ties at the k-th magnitude go to the HIGHER index;
              the ranking looks at |layer| BEFORE the residual is added
    values    v = layer + residual in the layer's compute type (float32 for float32 / float16 / bfloat16 layers, the 16-bit ones widened
              exactly; float64 for float64); no residual = zeros
    outputs   loc = the k indices, vals = v[loc], new residual = v with 0 at loc

A second ranking, `rank_keybits`, never looks at a float: it sorts the layers' bit patterns with the sign bit cleared, index as the
second key.  The two agree wherever there is no NaN, and the host test holds them to that.

A layer is a NumPy array of float32 / float64 / float16, or of uint16 for bfloat16 (its bit patterns: NumPy has no such type).

Two conditions on the inputs, asserted by every builder (conditions, not filters: no case is dropped):
  * no NaN in a layer: where a NaN ranks is unspecified;
  * no pair whose sum is NaN: an infinite value only meets a finite residual (the bit pattern of a generated NaN differs between x86
    and the GPU).  max + max = inf is allowed.
"""
import numpy as np

KINDS = ("f32", "f64", "f16", "bf16")
SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4097)                     # the host test's
GPU_SIZES = SIZES[:-1] + (4095, 4096, 4097, 9221)                               # the GPU test's


# ---------------------------------------------------------------------------------------------------------------- the reference
def kind_of(layer):
    return {np.dtype(np.float32): "f32", np.dtype(np.float64): "f64", np.dtype(np.float16): "f16", np.dtype(np.uint16): "bf16"}[layer.dtype]


def compute_dtype(kind):
    return np.dtype(np.float64 if kind == "f64" else np.float32)


def widen(layer):
    """The layer in its compute type (exact)."""
    layer = np.asarray(layer)
    if layer.dtype == np.uint16:                                                # bfloat16 bit patterns
        return (layer.astype(np.uint32) << np.uint32(16)).view(np.float32)
    if layer.dtype == np.float16:
        return layer.astype(np.float32)
    assert layer.dtype in (np.float32, np.float64)
    return layer


def rank_stable(x, k, mutate=None):
    """The k kept indices of a compute-type layer, ascending.  `mutate` bends the rule on purpose (the host test shows that the builders'
    inputs tell each bent rule from the right one): "ties_low" gives ties to the lower index."""
    mag = np.abs(x.astype(np.float64))
    if mutate == "ties_low":
        order = (x.size - 1 - np.argsort(mag[::-1], kind="stable"))
    else:
        order = np.argsort(mag, kind="stable")
    return np.sort(order[x.size - k:]).astype(np.uint32)


def rank_keybits(x, k, mutate=None):
    """The same selection from the bit patterns: ascending (bits & ~sign, index), the last k.  mutate = "keep_sign" leaves the sign bit in."""
    u = x.view(np.uint32 if x.dtype == np.float32 else np.uint64)
    if mutate != "keep_sign":
        u = u & ~(u.dtype.type(1) << u.dtype.type(8 * u.itemsize - 1))
    order = np.lexsort((np.arange(x.size), u))
    return np.sort(order[x.size - k:]).astype(np.uint32)


def topk_ref(layer, k, residual=None, rank=rank_stable, mutate=None):
    """-> (loc uint32[k] ascending, vals[k], new residual), the last two in the compute type.  mutate = "after_residual" ranks |x + r|."""
    x = widen(layer).reshape(-1)
    assert 0 <= k <= x.size and not np.isnan(x).any()
    r = np.zeros(x.size, dtype=x.dtype) if residual is None else np.asarray(residual).reshape(-1)
    assert r.dtype == x.dtype and r.size == x.size
    with np.errstate(over="ignore"):
        v = x + r
    assert v.dtype == x.dtype and not np.isnan(v).any()
    loc = rank(v if mutate == "after_residual" else x, k, mutate)
    new = v.copy()
    new[loc] = 0
    return loc, v[loc], new


def packed_ref(loc, bits):
    """`_to_bytes(loc, bits)` as little-endian uint64 limbs: the integer sum(loc[j] << bits (K - 1 - j))."""
    K = len(loc)
    big = 0
    for j, v in enumerate(loc):
        assert 0 <= int(v) < (1 << bits)
        big |= int(v) << (bits * (K - 1 - j))
    n_limbs = (K * bits + 63) // 64
    return np.frombuffer(big.to_bytes(8 * n_limbs, "little"), dtype=np.uint64).copy()


# ---------------------------------------------------------------------------------------------------------------- bit patterns
_F32_POOL = (0x00000000, 0x00000001, 0x000000ff, 0x00000100, 0x0000ff00, 0x00010000, 0x00ff0000, 0x007fffff, 0x00800000, 0x01000000,
             0x3f800000, 0x3f800001, 0x7f000000, 0x7f7fffff, 0x7f800000)
# 0xff and 0x01 at each of the eight byte positions below the sign (the top byte stops at 0x7f: the sign is not part of the key, and
# 0x7f with the next nibble below 0xf is still finite), max, inf
_F64_POOL = tuple([0x0, 0x3ff0000000000000, 0x3ff0000000000001, 0x0010000000000000, 0x000fffffffffffff, 0x7fefffffffffffff, 0x7ff0000000000000]
                  + [0xff << (8 * b) for b in range(7)] + [0x01 << (8 * b) for b in range(8)] + [0x7f << 56, 0x7fe0 << 48])
_F16_POOL = (0x0000, 0x0001, 0x00ff, 0x0100, 0x03ff, 0x0400, 0x0401, 0x3c00, 0x3c01, 0x7800, 0x7bff, 0x7c00)
_BF16_POOL = (0x0000, 0x0001, 0x007f, 0x0080, 0x0081, 0x00ff, 0x0100, 0x3f80, 0x3f81, 0x7f00, 0x7f7f, 0x7f80)
_FMT = {        # storage uint, sign bit, pool, (tops, lows): keys tops[i] | lows[j] with six distinct top digits of the WIDENED key
    "f32": (np.uint32, 31, _F32_POOL, ([t << 24 for t in (0x3f, 0x40, 0x3e, 0x00, 0x7f, 0x01)], [0x000000, 0x000001, 0x0000ff, 0x00ff00, 0x7f0000, 0x7fffff])),
    "f64": (np.uint64, 63, _F64_POOL, ([t << 56 for t in (0x3f, 0x40, 0x3e, 0x00, 0x7f, 0x01)],
                                       [0x0, 0x1, 0xff, 0xff00, 0xff0000, 0xff000000, 0xff << 32, 0xff << 40, 0xef << 48, 0xefffffffffffff])),
    # float16: exponent fields E whose float32 images have distinct top bytes, (E + 112) >> 1
    "f16": (np.uint16, 15, _F16_POOL, ([e << 10 for e in (15, 17, 5, 30, 1, 3)], [0x000, 0x001, 0x0ff, 0x100, 0x3ff])),
    "bf16": (np.uint16, 15, _BF16_POOL, ([t << 8 for t in (0x3f, 0x40, 0x3e, 0x00, 0x7f, 0x01)], [0x00, 0x01, 0x40, 0x7f])),
}
# how many lanes of a wave of 64 vote for each digit: fewer than 4, exactly 4, many more than 4; five or six heavy digits outlast the
# four rounds of the ballot loop
_LANE_COUNTS = {1: (64,), 3: (57, 4, 3), 4: (40, 16, 4, 4), 5: (30, 14, 10, 6, 4), 6: (25, 13, 10, 8, 5, 3)}


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def from_bits(kind, bits):
    """Storage array of a kind from unsigned bit patterns."""
    u = np.asarray(bits, dtype=_FMT[kind][0])
    return u if kind == "bf16" else u.view({"f32": np.float32, "f64": np.float64, "f16": np.float16}[kind])


def _signed(kind, bits, rng):
    ut, sb = _FMT[kind][0], _FMT[kind][1]
    u = np.asarray(bits, dtype=ut)
    return from_bits(kind, u | (rng.integers(0, 2, u.size).astype(ut) << ut(sb)))


def _of_values(kind, vals):
    """Storage array of a kind from float values that the kind holds exactly."""
    vals = np.asarray(vals, dtype=np.float64)
    if kind == "bf16":
        u = vals.astype(np.float32).view(np.uint32)
        assert not (u & np.uint32(0xffff)).any()
        return (u >> np.uint32(16)).astype(np.uint16)
    out = vals.astype({"f32": np.float32, "f64": np.float64, "f16": np.float16}[kind])
    assert np.array_equal(out.astype(np.float64), vals)
    return out


def residual_pool(kind, n, seed):
    """Residuals from {+-0, the smallest subnormal, -tiny, 1.0, max} of the compute type (all finite)."""
    ct = compute_dtype(kind)
    fi = np.finfo(ct)
    pool = np.array([0.0, -0.0, fi.smallest_subnormal, -fi.tiny, 1.0, fi.max], dtype=ct)
    return pool[_rng(seed).integers(0, pool.size, n)]


def default_ks(n):
    return sorted({0, 1, n // 2, n - 1, n} & set(range(n + 1)))


def _checked(layer, residual, ks):
    x = widen(layer)
    assert residual.dtype == x.dtype and residual.shape == x.shape == (layer.size,)
    assert not np.isnan(x).any(), "a NaN in the layer"
    with np.errstate(over="ignore"):
        assert not np.isnan(x + residual).any(), "a pair whose sum is NaN"
    assert all(0 <= k <= layer.size for k in ks)
    return layer, residual, list(ks)


# ---------------------------------------------------------------------------------------------------------------- the builders
def build_pool(kind, n, seed):
    """The kind's edge bit patterns (digits 0x00 / 0x01 / 0xff at each pass, subnormals, the normals' ends, inf), random signs."""
    rng = _rng(seed)
    pool = np.array(_FMT[kind][2], dtype=_FMT[kind][0])
    return _checked(_signed(kind, pool[rng.integers(0, pool.size, n)], rng), residual_pool(kind, n, seed + 1), default_ks(n))


def _build_digits(d):
    def build(kind, n, seed):
        """d distinct top digits, dealt to the lanes of every wave (a lane owns four consecutive elements) by _LANE_COUNTS[d]."""
        rng = _rng(seed)
        tops, lows = _FMT[kind][3]
        ut = _FMT[kind][0]
        lane_digit = np.repeat(np.arange(d), _LANE_COUNTS[d])
        lanes = (n + 3) // 4
        waves = (lanes + 63) // 64
        per_lane = np.concatenate([rng.permutation(lane_digit) for _ in range(waves)])[:lanes]
        top = np.array(tops, dtype=ut)[np.repeat(per_lane, 4)[:n]]
        low = np.array(lows, dtype=ut)[rng.integers(0, len(lows), n)]
        layer = _signed(kind, top | low, rng)
        u = widen(layer).view(np.uint32 if kind != "f64" else np.uint64)
        digits = np.unique((u >> u.dtype.type(8 * u.itemsize - 8)) & u.dtype.type(0x7f))
        assert digits.size <= d and (n < 256 or digits.size == d)
        return _checked(layer, residual_pool(kind, n, seed + 1), default_ks(n))
    build.__name__ = f"build_digits{d}"
    return build


def build_const(kind, n, seed):
    """One magnitude, random sign: every element ties."""
    rng = _rng(seed)
    return _checked(_signed(kind, _of_values(kind, np.full(n, 1.5)).view(_FMT[kind][0]), rng), residual_pool(kind, n, seed + 1), default_ks(n))


def build_zeros(kind, n, seed):
    """+-0 only."""
    rng = _rng(seed)
    return _checked(_signed(kind, np.zeros(n, dtype=_FMT[kind][0]), rng), residual_pool(kind, n, seed + 1), default_ks(n))


def build_lowbit(kind, n, seed):
    """{1.0, nextafter(1.0, 2.0)} of the kind, random sign: keys that agree in every digit but the last."""
    rng = _rng(seed)
    one = int(_of_values(kind, [1.0]).view(_FMT[kind][0])[0])
    bits = np.array([one, one + 1], dtype=_FMT[kind][0])[rng.integers(0, 2, n)]
    return _checked(_signed(kind, bits, rng), residual_pool(kind, n, seed + 1), default_ks(n))


def build_subnormal(kind, n, seed):
    """Multiples of the kind's smallest subnormal, with subnormal residuals of either sign in the compute type: the sums stay
    subnormal, cancel to zero, or cross into the normal range."""
    rng = _rng(seed)
    mant = {"f32": 23, "f64": 52, "f16": 10, "bf16": 7}[kind]
    top = (1 << mant) - 1
    m = np.array([0, 1, 2, 3, top // 2 + 1, top - 1, top], dtype=np.uint64)[rng.integers(0, 7, n)]
    rnd = rng.integers(0, top + 1, n, dtype=np.uint64)
    m = np.where(rng.integers(0, 2, n) == 1, m, rnd)
    layer = _signed(kind, m.astype(_FMT[kind][0]), rng)
    ct = compute_dtype(kind)
    cu = np.uint64 if ct == np.float64 else np.uint32
    cmant = 52 if ct == np.float64 else 23
    ctop = (1 << cmant) - 1
    x = widen(layer)
    rm = np.array([0, 1, 2, ctop // 2 + 1, ctop - 1, ctop], dtype=np.uint64)[rng.integers(0, 6, n)]
    rm = np.where(rng.integers(0, 3, n) == 0, np.abs(x).view(cu).astype(np.uint64) & np.uint64(ctop), rm)    # (cancels x where the signs differ and x is subnormal)
    res = (rm.astype(cu) | (rng.integers(0, 2, n).astype(cu) << cu(8 * ct.itemsize - 1))).view(ct)
    return _checked(layer, res, default_ks(n))


def riders_count(n):
    return (n + 36) // 37


def build_riders(kind, n, seed, ts=None):
    """Ties with riders: magnitude 0.5 everywhere, 3.0 at every 37th index, random sign; k = count(3.0) + t."""
    rng = _rng(seed)
    vals = np.full(n, 0.5)
    vals[::37] = 3.0
    cnt = riders_count(n)
    ts = ts if ts is not None else sorted({0, 1, (n - cnt) // 2, n - cnt} & set(range(n - cnt + 1)))
    ks = sorted(set(default_ks(n)) | {cnt + t for t in ts})
    return _checked(_signed(kind, _of_values(kind, vals).view(_FMT[kind][0]), rng), residual_pool(kind, n, seed + 1), ks)


BUILDERS = (build_pool, _build_digits(1), _build_digits(3), _build_digits(4), _build_digits(5), _build_digits(6), build_const, build_zeros,
            build_lowbit, build_subnormal, build_riders)


def all_tied(n, seed=5):
    """The tie-quota sweep's float32 layer: every element ties (magnitude 1.5, random sign); the residual makes every value distinct."""
    layer, _res, _ks = build_const("f32", n, seed)
    res = (np.arange(n) % 8191).astype(np.float32) * np.float32(0.25)
    return _checked(layer, res, [])[:2]
