"""Transport-free mirror of the adapter that drives the cipher in the reference
(federatedml/framework/homo/procedure/jzf_flashe_block.py): the `_Client` forwarders (:120-174) and
the arbiter's `dynamic_masking` cost model (:89-117).  Key exchange, uuid sync and the federation
transfer variables of the reference classes are control plane and are not reproduced; the PRP seed
is handed in directly.
"""
import functools
import math
import numbers
import operator
import os

import numpy as np

from . import _lib, interop
from .cipher import FlasheCipher, _CtxMask
from .quantize import ACIQ, QuantizingClient, _check_rng, _global_on_device, _loop_dtype, _rng_on_device

_RNG_RUN_MAX = 1 << 26          # draws per device call of quantize_encrypt (512 MiB of float64)

__all__ = ["dynamic_masking_choice", "FlasheClient", "FlasheCohort", "CohortPlan", "CohortUpload", "plan_cohort", "FlasheSparseCohort",
           "SparseCohortPlan", "SparseCohortEncoding", "SparseCohortUpload", "plan_sparse_cohort"]


def dynamic_masking_choice(masks, total, engine=None):
    """Arbiter.dynamic_masking's decision (jzf_flashe_block.py:92-112): "single" unless double masking would need strictly fewer PRF
    blocks.  single_cost = 2 * sum(len(mask)); double_cost = 2 * single_cost minus 2 per position shared by consecutive clients
    (their masks cancel).  The reference builds a one-hot vector of `total` entries per client and ANDs neighbours; the positions two
    clients share are the intersection of their location SETS, so nothing of size `total` is needed:
      * masks given as `(device buffer, length)` pairs -- strictly increasing uint32 lists already in HBM (what Sparsifier emits), with
        `engine` the Engine they live on: counted on the device (flashe_dynamic_masking_cost_dev), config-5 size in well under 1 ms;
      * host lists / arrays: sorted-set intersection of neighbours (np.intersect1d), O(k log k)."""
    if engine is not None and masks and all(isinstance(m, tuple) for m in masks):
        single_cost, double_cost = engine.dynamic_masking_cost_dev([m[0] for m in masks], [m[1] for m in masks])
        return "single" if single_cost <= double_cost else "double"
    single_cost = 2 * sum(len(m) for m in masks)
    double_cost = 2 * single_cost
    sets = []
    for m in masks:
        a = np.asarray(m, dtype=np.int64).reshape(-1)
        if a.size and (int(a.max()) >= total or int(a.min()) < -total):
            bad = int(a.max()) if int(a.max()) >= total else int(a.min())
            raise IndexError(f"index {bad} is out of bounds for axis 0 with size {total}")
        sets.append(np.unique(np.where(a < 0, a + total, a)))          # (one_hot[mask] = 1: a set; negative indices wrap as in NumPy)
    canceled = 0
    for i in range(len(sets) - 1):
        canceled += int(np.intersect1d(sets[i], sets[i + 1], assume_unique=True).size)
    double_cost -= canceled * 2
    return "single" if single_cost <= double_cost else "double"


def aggregate_sparse_uploads(engine, uploads, locations, total, device=True):
    """The arbiter's side of a sparse round on the device: what `Arbiter.expand_to_dense` (jzf_aggregator.py:150-165: a dense vector filled
    with the upload's LAST element -- the un-encrypted quantised zero -- and the other elements at the client's locations) followed by the
    reduce over the clients (`:419-430`) computes, in one pass without the C dense intermediates (flashe_sparse_aggregate_dev; strictly
    increasing location lists take the LDS-staged form).
      uploads   per client: a DeviceVector of k + 1 elements as FlasheClient.quantize_encrypt leaves it (it stays where it is), uint64 limbs
                [k + 1, L] or object ints [k + 1]
      locations per client: k sorted positions (host integers, or a device buffer of uint32)
    Returns the dense aggregate of `total` elements: a DeviceVector (device=True) or uint64 limbs [total, L]."""
    from .engine import DeviceBuffer, DeviceVector
    lim = engine.limbs
    vals, zeros, ks, locs, sorted_all = [], [], [], [], True
    for up, loc in zip(uploads, locations):
        if isinstance(up, DeviceVector):
            dv = up.widened(engine) if up.compact else up
            k = len(dv) - 1
            dv.wait_on(engine)
            z = dv.buf.download(np.uint64, (k + 1) * lim)[k * lim:]
            vals.append(dv.buf)
        else:
            a = np.asarray(up)
            if a.dtype == object:
                flat = a.reshape(-1)
                a = np.stack([(flat & (2 ** 64 - 1)).astype(np.uint64)] + ([((flat >> 64) & (2 ** 64 - 1)).astype(np.uint64)] if lim == 2 else []), axis=1)
            a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, lim)
            k = a.shape[0] - 1
            z = a[k]
            vals.append(engine.upload(a[:k]) if k else engine.alloc(16))
        zeros.append([int(v) for v in z])
        ks.append(k)
        if isinstance(loc, DeviceBuffer):
            locs.append(loc)
        else:
            la = np.asarray(loc, dtype=np.int64).reshape(-1)
            if la.size != k:
                raise ValueError(f"{la.size} locations for an upload of {k} values")
            sorted_all = sorted_all and bool(np.all(la[1:] > la[:-1]))
            locs.append(engine.upload(la.astype(np.uint32)) if k else engine.alloc(16))
    out = DeviceVector(engine, int(total))
    if total:
        engine.sparse_aggregate_dev(int(total), locs, ks, vals, zeros, out.buf, sorted_lists=sorted_all)
    return out.mark_ready() if device else out.to_host()


# ---- the client step's front-end rules, each stated once (FlasheClient's tensor step and both cohorts) ---------------------------------
_F32, _F64 = np.dtype(np.float32), np.dtype(np.float64)
_TENSOR_CODES = {"float32": _lib.TENSOR_F32, "float64": _lib.TENSOR_F64, "float16": _lib.TENSOR_F16, "bfloat16": _lib.TENSOR_BF16}


def _field_bits(element_bits, num_clients):
    """The bits of one batched field: the quantised value and room for the sum over the clients."""
    return element_bits + int(np.ceil(np.log2(num_clients)))


def _layer_source(eng, v, what):
    """One layer value -> (x, storage dtype code, NumPy dtype of its host copy, size, shape).  x is the ForeignArray of a framework device
    tensor, read where it lies (TypeError naming `what` for a dtype the kernels do not read), or the flat contiguous host array of anything
    else -- float32 and float64 as they are, every other dtype as float64."""
    if interop.is_foreign(v):
        fa = eng.foreign(v, what=what)
        if fa.dtype not in _TENSOR_CODES:
            raise TypeError(f"{what}: unsupported dtype {fa.dtype} (float32, float64, float16 or bfloat16)")
        return fa, _TENSOR_CODES[fa.dtype], _F64 if fa.dtype == "float64" else _F32, math.prod(fa.shape), fa.shape
    a = np.asarray(v)
    flat = np.ascontiguousarray(a).reshape(-1)
    if flat.dtype not in (np.float32, np.float64):
        flat = flat.astype(np.float64)
    return flat, _lib.TENSOR_F64 if flat.dtype == np.float64 else _lib.TENSOR_F32, flat.dtype, int(flat.size), a.shape


def _stage_host_layers(eng, row):
    """One client's layer sources -- flat host arrays, ForeignArrays, bare device pointers -- as (device pointers, keep).  The host arrays
    go up once into ONE buffer at 16-byte-aligned offsets (no buffer for a client without a host layer); keep holds that buffer and the
    owner of every ForeignArray: what must outlive the last kernel that reads the pointers."""
    offs, nbytes = {}, 0
    for li, x in enumerate(row):
        if isinstance(x, np.ndarray):
            offs[li] = nbytes
            nbytes += (x.nbytes + 15) & ~15
    keep = []
    if offs:
        xbuf = eng.alloc(max(nbytes, 16))
        for li, off in offs.items():
            xbuf.upload_at(off, row[li])
        keep.append(xbuf)
    ptrs = []
    for li, x in enumerate(row):
        if isinstance(x, np.ndarray):
            ptrs.append(xbuf.ptr + offs[li])
        elif isinstance(x, int):
            ptrs.append(x)
        else:
            ptrs.append(x.ptr)
            keep.append(x.keep)
    return ptrs, keep


def _round_alphas(q, sizes):
    """The alpha of every entry of q.layer_size_list for this round (ACIQ on the std history; 0 -> 0.1).  On first use `sizes` becomes the
    layer_size_list with the first round's expected mean / std (set_layer_size_list, jzf_quantize.py:380-392)."""
    if q.layer_size_list is None:
        q.layer_size_list = list(sizes)
        for _ in q.layer_size_list:
            q.past_layer_mean_list.append(q.expected_mean_for_first_round)
            q.past_layer_std_list.append(q.expected_std_for_first_round)
    aciq = ACIQ(q.element_bits)
    alphas = []
    for i in range(len(q.layer_size_list)):
        a = aciq.get_alpha_gaus_direct(q.past_layer_std_list[i])
        alphas.append(0.1 if a == 0 else a)
    return alphas


def _tensor_flags(hdt, alpha, normalize, mean):
    """(shift, flags) of a tensor-layer row whose host copy has NumPy dtype hdt: TENSOR_LOOP_F64 where NumPy's clip / scale arithmetic with
    alpha runs in float64 on a narrower layer; with normalize, shift = -mean (QuantizingClient._shift(layer, -mean)) under TENSOR_SHIFT, and
    TENSOR_SHIFT_WIDE where NumPy adds it to a float32 layer in float64."""
    flags, shift = 0, 0.0
    if hdt != np.float64 and _loop_dtype(hdt, alpha) == np.float64:
        flags |= _lib.TENSOR_LOOP_F64
    if normalize:
        shift = -mean
        flags |= _lib.TENSOR_SHIFT
        if hdt == np.float32 and _loop_dtype(hdt, shift) == np.float64:
            flags |= _lib.TENSOR_SHIFT_WIDE
    return float(shift), flags


def _check_degree(v, what):
    """The aggregator's degree / the arbiter's sum of degrees (jzf_aggregator.py:676, :380): None, or a positive finite real number --
    anything else is a ValueError (the reference's `if degree:` takes 0 for "no degree" and then divides by it, :902)."""
    if v is None:
        return None
    ok = isinstance(v, (numbers.Real, np.floating, np.integer)) and not isinstance(v, (bool, np.bool_))
    try:
        f = float(v) if ok else 0.0
    except OverflowError:
        f = math.inf
    if not ok or not math.isfinite(f) or not f > 0:
        raise ValueError(f"{what} must be a positive finite real number (None: no scaling), got {v!r}")
    return v


def _layers_of(w):
    """The {name: layer} dict of a Weights-like object or of a plain dict."""
    return w._weights if hasattr(w, "_weights") else w


def _stage_scaled(eng, items):
    """`weights *= degree` (jzf_aggregator.py:676) and normalize (jzf_quantize.py:542-547) of device-resident layers in ONE streaming
    pass (flashe_stage_layers_dev).  items: (pointer, storage dtype code, NumPy dtype of the host copy, size, degree or None, alpha,
    mean or None) per layer -- one model's, or every client's of a cohort.  Every step takes the dtype the running NumPy gives
    `array <op> scalar` there: the multiply makes a new array (a float32 layer becomes float64 under an np.float64 degree), the shift is
    in place, and the result is stored in the dtype the clip / scale arithmetic with alpha runs in.  Returns ([(pointer, F32 / F64 code)]
    -- a layer that needs nothing is read where it lies --, the scratch buffer or None)."""
    plans, nbytes = [], 0
    for ptr, code, hdt, size, degree, alpha, mean in items:
        cur, flags, scale, shift = np.dtype(hdt), 0, 1.0, 0.0
        if degree is not None:
            nxt = _loop_dtype(cur, degree)
            if nxt not in (_F32, _F64):
                raise TypeError(f"degree {degree!r} makes a {cur} layer {nxt}: float32 and float64 are what the kernels compute in")
            flags |= _lib.STAGE_SCALE | (_lib.STAGE_SCALE_WIDE if cur == _F32 and nxt == _F64 else 0)
            cur, scale = nxt, float(degree)
        if mean is not None:
            shift = -mean
            flags |= _lib.STAGE_SHIFT | (_lib.STAGE_SHIFT_WIDE if cur == _F32 and _loop_dtype(cur, shift) == _F64 else 0)
        out64 = cur == _F64 or _loop_dtype(cur, alpha) == _F64
        direct = not flags and code == (_lib.TENSOR_F64 if out64 else _lib.TENSOR_F32)
        if out64:
            flags |= _lib.STAGE_OUT_F64
        at = None
        if not direct:
            at = nbytes
            nbytes += (size * (8 if out64 else 4) + 15) & ~15
        plans.append((ptr, code, size, scale, float(shift), flags, out64, at))
    if all(p[7] is None for p in plans):
        return [(p[0], p[1]) for p in plans], None
    buf = eng.alloc(max(nbytes, 16))
    eng.stage_layers_dev([(ptr, buf.ptr + at, size, scale, shift, code, flags) for ptr, code, size, scale, shift, flags, _o, at in plans
                          if at is not None])
    return [(ptr, code) if at is None else (buf.ptr + at, _lib.TENSOR_F64 if out64 else _lib.TENSOR_F32)
            for ptr, code, _size, _sc, _sh, _fl, out64, at in plans], buf


def _size(shape):
    """The number of values of a layer of that shape, as a Python int (it reaches ctypes)."""
    return int(math.prod(shape))


def _draws(eng, count, rng=None):
    """The next `count` stochastic-rounding draws of NumPy's global stream as a device buffer: generated on the device
    (_global_on_device), else drawn on the host and uploaded.  rng (a Generator): its next `count` draws instead -- on the device under
    _rng_on_device (Philox, PCG64, PCG64DXSM), else rng.random(count) uploaded."""
    if rng is not None:
        call = _rng_on_device(eng, rng, count)
        return getattr(eng, call)([rng], [count]) if call else eng.upload(rng.random(count))
    return eng.numpy_random_dev(count) if _global_on_device(eng, count) else eng.upload(np.random.random(count))


def _skip_draws(count, rng=None):
    """`count` draws taken and dropped (a refusal that the call-by-call step raises after its quantiser has drawn): from rng, else from
    NumPy's global stream."""
    for at in range(0, count, _RNG_RUN_MAX):
        (np.random.random if rng is None else rng.random)(min(_RNG_RUN_MAX, count - at))


def _rng_kw(rng):
    """rng= as a keyword for a forwarded call: absent without one, so that rng=None makes exactly the calls it always made."""
    return {} if rng is None else {"rng": rng}


def _client_rng(rng, ci):
    """Client ci's Generator of a cohort's rng= (one Generator for all, or one per client), None without."""
    return rng[ci] if isinstance(rng, list) else rng


_DRAW_CALL_SEGMENTS = {"philox_random_dev": "PHILOX_MAX_SEGMENTS", "pcg64_random_dev": "PCG64_MAX_SEGMENTS"}    # the segments a call holds


def _cohort_rng_draws(eng, C, per_client, rng):
    """_cohort_draws from the caller's generators: one Generator gives ONE stretch of C per_client draws, a list client c's stretch from
    rng[c].  The stretches that run on the device (_rng_on_device) are grouped by the call that takes them: every kind -- Philox, the
    PCG64 family -- is ONE launch of a segment per stretch whatever C is; the others are rng.random(...) on the host, uploaded in runs
    of at most _RNG_RUN_MAX draws."""
    du = eng.alloc(max(8 * C * per_client, 16))
    stretches = [(rng[ci], ci * per_client, per_client) for ci in range(C)] if isinstance(rng, list) else [(rng, 0, C * per_client)]
    dev = {}                                          # the device call -> its stretches
    for g, first, count in stretches:
        call = _rng_on_device(eng, g, count)
        if call:
            dev.setdefault(call, []).append((g, first, count))
            continue
        for at in range(first, first + count, _RNG_RUN_MAX):
            du.upload_at(8 * at, g.random(min(_RNG_RUN_MAX, first + count - at)))
    for call, mine in dev.items():
        most = getattr(eng, _DRAW_CALL_SEGMENTS[call])
        for at in range(0, len(mine), most):                                            # (a cohort holds at most 128 clients: one launch)
            part = mine[at:at + most]
            getattr(eng, call)([g for g, _f, _c in part], [c for _g, _f, c in part], out=du, offsets=[f for _g, f, _c in part])
    return du


def _cohort_draws(eng, C, per_client, seeds, rng=None):
    """The stochastic-rounding draws of C clients, client-major, as a device buffer: client c's are draws [c per_client, (c + 1) per_client).
    From the global stream (seeds=None) they are ONE stretch of C per_client draws -- the clients draw one after the other -- generated in
    device calls of at most _RNG_RUN_MAX draws whatever client they belong to (the jump-ahead of a device call is paid per call, not per
    client); with seeds every client's stretch starts at its own seed.  On the device under quantize_encrypt's rule (_global_on_device, per
    call), else drawn on the host and uploaded.  rng: the caller's generators instead (_cohort_rng_draws)."""
    if rng is not None:
        return _cohort_rng_draws(eng, C, per_client, rng)
    du = eng.alloc(max(8 * C * per_client, 16))
    for seed, first, count in ([(None, 0, C * per_client)] if seeds is None else [(seeds[ci], ci * per_client, per_client) for ci in range(C)]):
        if seed is not None:
            np.random.seed(seed)
        for at in range(first, first + count, _RNG_RUN_MAX):
            tot = min(_RNG_RUN_MAX, first + count - at)
            if _global_on_device(eng, tot):
                eng.numpy_random_dev(tot, out=du.ptr + 8 * at)
            else:
                du.upload_at(8 * at, np.random.random(tot))
    return du


# Is the inline form the default of a shape class (compact layout?, every client's stream starts at a Philox block?) -- the round-9 rule:
# only where its median beat the buffer form's by more than the larger of the two spreads.  FLASHE_INLINE_DRAWS=1 forces it elsewhere.
_INLINE_DRAWS_DEFAULT = {(False, True): True, (False, False): True, (True, True): True, (True, False): True}


def _draws_aligned(rng, C, n):
    """Does every client's stretch start at a block of its Philox stream (a run of four values is then ONE block)?  A list: every
    generator's buffer is fresh or exhausted (buffer_pos 4, or 0 set by hand); one shared generator: that, and n % 4 == 0 or one client."""
    if isinstance(rng, list):
        return all(int(g.bit_generator.state["buffer_pos"]) in (0, 4) for g in rng)
    return int(rng.bit_generator.state["buffer_pos"]) in (0, 4) and (n % 4 == 0 or C <= 1)


# The same rule for a BATCHED job that asked for the inline form (FlasheCohort(inline_draws=True)): (values per element, ONE Generator
# shared by the clients?, every client's stream starts at a Philox block?) -> inline by default.  A class that is not listed -- one that
# lost the measurement (tests/perf/prepared_cohort_batched_inline_draws.py) or was not measured -- keeps the buffer.  Measured
# (profiles/r34_prepared_cohort_batched_inline_draws.log): one shared generator at a misaligned length -- the buffer form's draw launch
# is slow there -- wins at six and seven values per element by 34 - 82 % against spreads of 6 - 11 %; a list of fresh generators
# (aligned) loses or ties (A / B 0.67 - 1.04: the launch is bound by its Philox rounds), and five values per element lost both ways
# on a hundred small models (A / B 0.25 - 0.38).  Not measured, so not listed: a list of generators at odd positions, one shared
# generator whose clients all start at a block, and every run-time bs.
_INLINE_BATCHED_DEFAULT = {(6, True, False): True, (7, True, False): True}


def _batched_draws_class(rng, bs, C, n):
    """The key of a batched round in _INLINE_BATCHED_DEFAULT."""
    return (int(bs), not isinstance(rng, list), _draws_aligned(rng, C, n))


def _inline_draws(eng, rng, batched, compact=False, C=1, n=0, inline_batched=False, bs=0):
    """Does a "prepared-cohort" round generate its draws INSIDE the online launch (eng.quantize_combine_cohort_philox_dev: no draw
    buffer, one launch less)?  Every (present) client's Generator over np.random.Philox, FLASHE_DEVICE_RNG not 0, an engine that has the
    call, and FLASHE_INLINE_DRAWS (the A/B switch, read per call): 0 never, 1 always, unset the default of the round's shape class
    (_INLINE_DRAWS_DEFAULT).  No DEVICE_RNG_MIN threshold: there is no extra launch to amortise.  A batched job (bs values per element, n
    values per client) reads the draw buffer unless the cohort asked for the inline form (inline_batched: FlasheCohort(inline_draws=True))
    and the engine has eng.quantize_batch_combine_cohort_philox_dev -- a lane of that launch owns four elements, so that no Philox
    block is computed twice; its class defaults are _INLINE_BATCHED_DEFAULT's."""
    if rng is None or not hasattr(eng, "quantize_batch_combine_cohort_philox_dev" if batched else "quantize_combine_cohort_philox_dev"):
        return False
    if batched and not inline_batched:
        return False
    switch = os.environ.get("FLASHE_INLINE_DRAWS", "")
    if os.environ.get("FLASHE_DEVICE_RNG", "1") == "0" or switch == "0":
        return False
    gens = rng if isinstance(rng, list) else [rng]
    if len(gens) > eng.PHILOX_MAX_SEGMENTS or not all(isinstance(g.bit_generator, np.random.Philox) for g in gens):
        return False
    if switch == "1":
        return True
    if batched:
        return _INLINE_BATCHED_DEFAULT.get(_batched_draws_class(rng, bs, C, n), False)
    return _INLINE_DRAWS_DEFAULT[(bool(compact), _draws_aligned(rng, C, n))]


# The same rule for the generators of the PCG64 family (np.random.default_rng's) in a cohort made with inline_draws="any": compact layout?
# -> inline by default, and only where the inline median beat the buffer form's by more than the larger of the two spreads in EVERY case
# of the layout.  Measured (tests/perf/prepared_cohort_pcg64_inline_draws.py, profiles/r35_prepared_cohort_pcg64_inline_draws.log: ten
# clients of 1e7 and 25,557,032 values, PCG64 and PCG64DXSM, one shared generator and a list): int_bits 128 wins by 18 - 25 % against
# spreads of 2 - 6 %, int_bits 20 compact by 35 - 75 % against 10 - 16 %.
_INLINE_PCG64_DEFAULT = {False: True, True: True}


def _inline_pcg64_draws(eng, rng, batched, compact=False):
    """_inline_draws for generators over np.random.PCG64 or np.random.PCG64DXSM (eng.quantize_combine_cohort_pcg64_dev), asked only by a
    cohort made with inline_draws="any": an un-batched round (the launch has no batched form), every (present) client's Generator of ONE
    of the two variants -- the launch's lanes share one jump --, at most eng.PCG64_MAX_SEGMENTS of them, FLASHE_DEVICE_RNG not 0, an engine
    that has the call, and FLASHE_INLINE_DRAWS: 0 never, 1 always, unset the default of the layout (_INLINE_PCG64_DEFAULT)."""
    if rng is None or batched or not hasattr(eng, "quantize_combine_cohort_pcg64_dev"):
        return False
    switch = os.environ.get("FLASHE_INLINE_DRAWS", "")
    if os.environ.get("FLASHE_DEVICE_RNG", "1") == "0" or switch == "0":
        return False
    gens = rng if isinstance(rng, list) else [rng]
    if len(gens) > eng.PCG64_MAX_SEGMENTS:
        return False
    if not any(all(type(g.bit_generator) is kind for g in gens) for kind in (np.random.PCG64, np.random.PCG64DXSM)):
        return False
    if switch == "1":
        return True
    return _INLINE_PCG64_DEFAULT[bool(compact)]


class FlasheClient(object):
    """`jzf_flashe_block._Client` without the transport: holds a FlasheCipher and forwards to it with the
    reference's method names, so `JZFWeights.encrypted(cipher)` / `.decrypted(cipher)`
    (jzf_weights.py:334-338) can be handed this object unchanged."""

    def __init__(self, args, device=0, stream=None):
        """stream (new): a framework's hipStream_t as an int -- the cipher's engine runs on it (FlasheCipher(stream=...))."""
        q = args['quantize']
        self.int_bits = q['int_bits']
        self.batch = q.get('batch')
        self.element_bits = q.get('element_bits')
        self.padding = q.get('padding')
        self.secure = q.get('secure')
        self.precompute = args.get('precompute', {}).get('enable', False)
        if self.precompute:
            self.num_params = args['precompute']['num_params']
        self.mask = args.get('mask', 'double')
        self.cipher = None
        self.quantizer = None
        self.shape_dict = None           # layer shapes of the flattened model (what the aggregator-side Client keeps, jzf_aggregator.py:648)
        self.fuse = True                 # False: quantize_encrypt / decrypt_unquantize run the reference's sequence call by call
        self.degree = None               # the degree the last quantize_encrypt took (jzf_aggregator.py:676): decrypt_unquantize's default
        self._device = device
        self._stream = stream

    def create_cipher(self, idx, num_clients, prp_seed):
        """What Guest/Host.create_cipher leave behind (:193-244, :287-326): a keyed cipher that knows its
        client index and, with precompute enabled, the masks of iteration 0."""
        self.cipher = FlasheCipher(self.int_bits, device=self._device, stream=self._stream)
        self.cipher.idx = idx
        self.cipher.set_num_clients(num_clients)
        self.cipher.generate_prp_seed(prp_seed)
        if self.precompute:
            self.cipher.set_num_params(self.num_params)
            self.cipher.prepare_encrypt()
        # the quantiser the reference creates right after the cipher (:229-238, :311-320); num_clients arrives over the wire there
        self.quantizer = QuantizingClient(self.int_bits, None, None, self.batch, self.element_bits, self.padding, self.secure,
                                          device=self._device)
        self.quantizer.num_clients = num_clients
        return self.cipher

    def dynamic_masking(self, choice, masks):
        """Client side of the arbiter hint (:185-191, :278-285)."""
        if not self.mask == "dynamic":
            return
        self.cipher.masking_scheme = choice
        self.cipher.masks = masks

    def encrypt(self, plaintext, device=None):
        """device (new): True keeps the ciphertext in HBM and returns a DeviceVector, see FlasheCipher.encrypt."""
        return self.cipher.encrypt(plaintext, device=device)

    def decrypt(self, ciphertext, device=None):
        return self.cipher.decrypt(ciphertext, device=device)

    def get_idx_list(self):
        return self.cipher.get_idx_list()

    def set_idx_list(self, idx_list):
        self.cipher.set_idx_list(raw_idx_list=idx_list, mode="decrypt")

    def set_iter_index(self, iter_index):
        self.cipher.set_iter_index(iter_index)
        self.quantizer.set_iter(iter_index)

    # the quantiser forwarders of _Client / Guest / Host (:159-163, :254-264)
    def quantize(self, weights, rng=None):
        rng = _check_rng(rng)
        if self.quantizer.layer_size_list is None:
            self.quantizer.set_layer_size_list(weights)
        return self.quantizer.quantize(weights, **_rng_kw(rng))

    def normalize(self, weights):
        if self.quantizer.layer_size_list is None:
            self.quantizer.set_layer_size_list(weights)
        return self.quantizer.normalize(weights)

    def unquantize(self, weights):
        return self.quantizer.unquantize(weights)

    def unnormalize(self, weights):
        return self.quantizer.unnormalize(weights)

    # ---- flatten / unflatten: Client.flatten_weights / unflatten_weights of the aggregator (jzf_aggregator.py:625-671) ------------------
    def flatten_weights(self, weights):
        """Client.flatten_weights (jzf_aggregator.py:625-650): the layers, in walking order, become ONE vector under the first key; the
        shapes (all but the sparse job's 'zzz' layer) are kept in `self.shape_dict` for unflatten_weights.  A reference job encrypts
        this vector, so PRF counters and the int_bits <= 64 chunking run across the layers."""
        parts, shape_dict, first_k = [np.array([])], {}, None
        for k in list(weights.walking_order):
            if first_k is None:
                first_k = k
            layer = np.asarray(weights._weights[k])
            if k != "zzz":
                shape_dict[k] = layer.shape
            parts.append(layer.flatten())
            del weights._weights[k]
        self.shape_dict = shape_dict
        if first_k is not None:
            weights._weights[first_k] = np.concatenate(parts)
        weights.walking_order = sorted(weights._weights.keys(), key=str)
        return weights

    def unflatten_weights(self, weights):
        """Client.unflatten_weights (jzf_aggregator.py:652-671): cut the one vector back into `self.shape_dict`'s layers."""
        only_key = weights.walking_order[0]
        flat = weights._weights[only_key]
        for k, shape in self.shape_dict.items():
            size = _size(shape)
            weights._weights[k] = flat[:size].reshape(shape)
            flat = flat[size:]
        weights.walking_order = sorted(weights._weights.keys(), key=str)
        return weights

    # ---- the client step with nothing on the host in between (new) ------------------------------------------------------------
    def _fusable(self, weights=None):
        c = self.cipher
        if not (self.fuse and c.prp_seed is not None and hasattr(c.engine, "quantize_encrypt_model_dev")):
            return False
        c._reconcile_prepared()
        if weights is None or "zzz" not in weights._weights:
            return c.masks is None and self._prepared_mode(c.next_iter_encrypt_prepared) is not False
        if c.next_iter_encrypt_prepared:
            return False
        # the sparse job: compact layers + the sparsifier's trailing one-value layer (the masks a previous round's decrypt left in the
        # cipher do not touch the encrypt)
        order = list(weights.walking_order)
        return not self.batch and len(order) > 1 and order[-1] == "zzz" and np.size(weights._weights["zzz"]) == 1

    def _prepared_mode(self, prep):
        """What the fused step does with a next_iter_*_prepared dict (the reference's mask cache, jzf_flashe.py:599-666):
        None   = empty;
        "ctx"  = double mask, both entries handles of masks the engine's ctx holds: the fused launches read them and consume the cache;
        "single" = single mask: the reference does not read the cache, it only drops one entry (:452-454, :533-535);
        False  = anything else (plain arrays a caller assigned): the call-by-call step."""
        c = self.cipher
        if not prep:
            return None
        if c.masking_scheme != "double":
            return "single"
        ok = (isinstance(prep, dict) and isinstance(prep.get('add'), _CtxMask) and isinstance(prep.get('minus'), _CtxMask)
              and hasattr(c.engine, "quantize_encrypt_prepared_model_dev"))
        return "ctx" if ok else False

    def _encrypt_done(self, mode):
        """The entries the call-by-call encrypt deletes (:452-454, :483-486); the ctx has consumed its cache in the last launch."""
        c = self.cipher
        if mode == "ctx":
            del c.next_iter_encrypt_prepared['add'], c.next_iter_encrypt_prepared['minus']
            c._ctx_holds &= ~c.engine.PREPARED_ENCRYPT
        elif mode == "single":
            c.next_iter_encrypt_prepared.pop('add', None)

    def _decrypt_done(self, mode):
        """The same for the decrypt (:533-535, :573-580): the encrypt cache of the next round is not touched."""
        c = self.cipher
        if mode == "ctx":
            for d in (c.next_iter_decrypt_prepared, c.next_iter_decrypt_prepared_idx):
                d.pop('add', None)
                d.pop('minus', None)
            c._ctx_holds &= ~c.engine.PREPARED_DECRYPT
        elif mode == "single":
            c.next_iter_decrypt_prepared.pop('minus', None)

    def _refuse_prepared_len(self, n_ct, n_values, rng=None):
        """An encrypt cache of another length: the call-by-call step's ValueError (cipher._check_prepared_len), raised where that step
        raises it -- after its quantiser has drawn one value of NumPy's stream (of rng) per model value.  The cache stays."""
        c = self.cipher
        cache = c.next_iter_encrypt_prepared['add']
        if len(cache) == n_ct:
            return
        _skip_draws(n_values, rng)
        c._check_prepared_len(cache, n_ct)

    def quantize_encrypt(self, weights, device=True, normalize=False, rng=None, degree=None):
        """degree (new): `weights *= degree` first (jzf_aggregator.py:676, the client's sample count times aggregate_every_n_epoch): every
        layer but the sparse job's 'zzz' becomes a NEW array `layer * degree` in the dtype NumPy gives that product (a float32 layer stays
        float32 under a Python number and becomes float64 under an np.float64), the caller's arrays and tensors are never written; host
        layers are multiplied on the host, framework tensors in the stage pass that normalisation pays anyway
        (flashe_stage_layers_dev).  None: no scaling; zero, negative, non-finite or not a real number: ValueError before anything is
        touched.  The client remembers it for decrypt_unquantize.

        rng (new): a np.random.Generator the stochastic-rounding draws come from -- the result is that of the same call with every
        np.random.random(k) replaced by rng.random(k), the sparse job's 'zzz' draw included (the next draw of the same generator); NumPy's
        global stream is neither read nor advanced.  Over np.random.Philox, np.random.PCG64 (np.random.default_rng) or
        np.random.PCG64DXSM, stretches of DEVICE_RNG_MIN draws or more are generated on the device (flashe_philox_random_dev,
        flashe_pcg64_random_dev) and the advanced state is put back into the generator; any other generator draws on the host.  Anything that is not a Generator: TypeError, before anything is touched.

        normalize (new): QuantizingClient.normalize first (`-= past_layer_mean_list[i]`, jzf_quantize.py:542-547).  Layers may also be
        a framework's float DEVICE tensors (float32 / float64 / float16 / bfloat16, DLPack or __cuda_array_interface__), mixed with host
        layers: they are read where they lie (see _quantize_encrypt_tensors), no layer byte crosses PCIe.

        What Client.secure_aggregate does between "begin encoding" and "end encryption" (jzf_aggregator.py:721-743):
        `self.quantize(weights)` -> `flatten_weights` -> [sparse job: strip the trailing quantised zero] -> `weights.encrypted(self)`
        -> [re-append it] -- QuantizingClient.quantize (jzf_quantize.py:394-491), then ONE cipher.encrypt over the flattened model
        (jzf_weights.py:334-338 -> jzf_flashe_block.py:142-150), so that element j of the model is masked with PRF counter j whatever
        layer it sits in -- with no host round trip in between: every layer goes up once as it is (4 or 8 bytes per value) into one flat
        device buffer, the stochastic-rounding draws of the whole model are generated on the device from NumPy's own stream (small
        models: drawn on the host), and ONE launch quantises and encrypts (flashe_quantize_encrypt_model_dev: per-layer alpha from a
        device table).  Bit-identical to the reference's sequence with the same seed (tests/golden/clientstep.json).
        The result has the reference's form: one key (the first of the walking order) holding the flattened ciphertext -- a
        DeviceVector (device=True: it stays in HBM for `aggregate`) or uint64 limbs [n, L]; `self.shape_dict` keeps the shapes for
        `decrypt_unquantize`.  BATCHED jobs ("batch": true, several quantised values per ciphertext element, every layer padded to whole
        elements on its own: jzf_quantize.py:436-451, :162-185) are two launches: quantise + batch of the whole model
        (flashe_quantize_batch_model_dev), then the encrypt of the flattened batched vector.  The SPARSE job (compact layers from
        `Client.sparsify` plus the one-value 'zzz' layer, jzf_aggregator.py:717-743) is the same one launch over the compact layers; the
        'zzz' value is quantised on the host with the draw that follows theirs (alpha 1.0, jzf_quantize.py:433-435) and appended
        UN-encrypted: the result holds n + 1 elements.  PRECOMPUTED encrypt masks (precompute jobs: the handles prepare_encrypt leaves in
        next_iter_encrypt_prepared) are added by the same launches in place of the PRF streams -- no AES; the batched job's quantise +
        batch + encrypt becomes one launch -- and consumed as the call-by-call encrypt consumes them; a single-mask cipher ignores them
        and drops 'add' as the reference does.  Batched sparse jobs, sparse jobs with a cache and masks a caller assigned as plain arrays
        take the same sequence call by call on the host and return object arrays like the reference."""
        q = self.quantizer
        rng = _check_rng(rng)
        self.degree = _check_degree(degree, "degree")
        if any(interop.is_foreign(weights._weights[k]) for k in weights.walking_order):
            return self._quantize_encrypt_tensors(weights, device, normalize, rng, degree)
        if degree is not None:
            for k in weights.walking_order:
                if k != "zzz":                                               # (the sparsifier creates it after :676)
                    weights._weights[k] = np.asarray(weights._weights[k]) * degree
        if normalize:
            self.normalize(weights)
        if q.layer_size_list is None:
            q.set_layer_size_list(weights)
        if not self._fusable(weights):
            sparse = "zzz" in weights._weights
            weights = self.flatten_weights(self.quantize(weights, **_rng_kw(rng)))
            k0 = weights.walking_order[0]
            flat = weights._weights[k0]
            if sparse:                                                       # jzf_aggregator.py:735-743
                zero_quantized, flat = flat[-1], flat[:-1]
            ct = self.cipher.encrypt(flat)
            weights._weights[k0] = np.append(ct, [zero_quantized]) if sparse else ct
            return weights
        return self._encrypt_tail(weights, device, *self._host_front_end(weights), rng=rng)

    def _host_front_end(self, weights):
        """The fused step's front end for host layers (normalised on the host already, layer_size_list set): every layer goes up once,
        widened on the host to the dtype NumPy's clip / scale arithmetic with its alpha runs in, and the launches are the *_model_dev entry
        points over 4-field rows (start -- batched: size --, pointer, alpha, is float64).  Returns _encrypt_tail's arguments."""
        q, c = self.quantizer, self.cipher
        eng = c.engine
        mode = self._prepared_mode(c.next_iter_encrypt_prepared)
        alphas = _round_alphas(q, q.layer_size_list)
        q.r_max_list, q.alpha_list = [], []
        c.set_idx_list(mode="encrypt")
        order, zzz = list(weights.walking_order), None
        if "zzz" in weights._weights:                       # (_fusable: it closes the walking order)
            zzz = np.asarray(weights._weights["zzz"])
            order = order[:-1]
        host, sizes, starts, shape_dict, n = [], [], [], {}, 0
        for li, k in enumerate(order):
            alpha = alphas[li]
            q.r_max_list.append(alpha * q.num_clients)
            q.alpha_list.append(alpha)
            flat, _code, hdt, size, shape_dict[k] = _layer_source(eng, weights._weights[k], f"layer {k!r}")
            want = _loop_dtype(hdt, alpha)                         # the dtype NumPy's clip / scale arithmetic runs in
            host.append(flat if hdt == want else flat.astype(want))
            sizes.append(size)
            starts.append(n)
            n += size
        ptrs, keep = _stage_host_layers(eng, host)
        rows = [(sizes[li] if self.batch else starts[li], ptrs[li], q.alpha_list[li], host[li].dtype == np.float64) for li in range(len(order))]
        launch = (eng.quantize_encrypt_model_dev, eng.quantize_encrypt_prepared_model_dev, eng.quantize_batch_model_dev,
                  eng.quantize_batch_encrypt_prepared_model_dev)
        return mode, order, zzz, sizes, starts, shape_dict, rows, launch, keep

    def _encrypt_tail(self, weights, device, mode, order, zzz, sizes, starts, shape_dict, rows, launch, keep, hold=None, normalize=False,
                      rng=None):
        """The fused step behind either front end: the draws, the launches and the result.  `rows` are the layers `order` (sizes, starts,
        shape_dict) as the four entry points in `launch` -- un-batched online and prepared, batched online and prepared -- read them; mode
        is _prepared_mode of the encrypt cache; zzz the sparse job's trailing value (host) or None; keep what the launches read: it lives to
        the end of the call.  The tensor front end also passes hold (the owners of the caller's tensors: held on the engine until the
        launches have finished) and normalize (the 'zzz' value is still to be normalised -- the host front end has normalised the whole
        model); rng the Generator the draws come from (None: NumPy's global stream)."""
        from . import cipher as _cipher_mod
        from .engine import DeviceVector
        q, c = self.quantizer, self.cipher
        eng, n = c.engine, sum(sizes)
        online, prepared, batch, batch_prepared = launch
        scheme = 1 if c.masking_scheme == "double" else 0
        if self.batch:
            # quantise + batch of the whole model in ONE launch (per-layer alpha, per-layer zero padding), then the encrypt of the flattened
            # batched vector: the draws are one stretch of NumPy's stream over all VALUES in walking order
            field_bits = _field_bits(q.element_bits, q.num_clients)
            bs = self.int_bits // field_bits
            q.shape_list = [shape_dict[k] for k in order]
            n_elems = sum((s_ + bs - 1) // bs for s_ in sizes)
            if mode == "ctx":
                self._refuse_prepared_len(n_elems, n, rng)
            du = _draws(eng, n, rng) if n else eng.alloc(16)
            ct = DeviceVector(eng, n_elems)
            if mode == "ctx":                   # quantise + batch + the prepared masks: one launch, no AES
                batch_prepared(rows, q.element_bits, field_bits, du, n_elems, ct.buf)
            else:
                pt = eng.alloc_vec(max(n_elems, 1))
                batch(rows, q.element_bits, field_bits, du, n_elems, pt)
                if n_elems:
                    eng.encrypt_dev(c.iter_index, c.idx, scheme, n_elems, _cipher_mod.N_JOBS, pt, eng.limbs, ct.buf)
            shape_dict = {k: ((s_ + bs - 1) // bs,) for k, s_ in zip(order, sizes)}      # the batched layers are 1-D (:448)
        else:
            # the draws of consecutive layers are ONE stretch of NumPy's stream (np.random.random(layer.shape) per layer in walking order,
            # jzf_quantize.py:55-67 under :417-462), i.e. flat element j takes draw j: a run of whole layers is drawn by one device call and
            # quantised + encrypted by one launch over its range.  Runs are capped so the draws of a huge model stay bounded.  With the ctx's
            # prepared masks the launches add them in place of the PRF streams; the run that ends the vector consumes them.
            if mode == "ctx":
                self._refuse_prepared_len(n, n, rng)
            ct = DeviceVector(eng, n + (1 if zzz is not None else 0))
            at = 0
            while at < len(order):
                end, tot = at, 0
                while end < len(order) and (end == at or tot + sizes[end] <= _RNG_RUN_MAX):
                    tot += sizes[end]
                    end += 1
                if tot:
                    du, first = _draws(eng, tot, rng), starts[at]
                    if mode == "ctx":
                        prepared(n, first, tot, rows, q.element_bits, du, ct.ptr + first * eng.limbs * 8)
                    else:
                        online(c.iter_index, c.idx, scheme, n, _cipher_mod.N_JOBS, first, tot, rows, q.element_bits, du,
                               ct.ptr + first * eng.limbs * 8)
                at = end
            if mode == "ctx" and n == 0:
                eng.prepared_discard(eng.PREPARED_ENCRYPT)          # (nothing to add the masks to: consumed all the same)
        self._encrypt_done(mode)
        if hold is not None:
            eng.hold(hold)
        if zzz is not None:
            # the trailing layer: (normalised with its own mean, then) the next draw of the stream, alpha 1.0, not encrypted (:735-743
            # strips it before and re-appends it after)
            from .quantize import _as_object, _static_quantize_padding_asymmetric
            if normalize:
                d, a = q._shift(zzz, -q.past_layer_mean_list[len(order)])
                zzz = d.download(a.dtype, a.size).reshape(a.shape)
            flat = zzz.flatten()
            want = _loop_dtype(flat.dtype, 1.0)
            if flat.dtype != want:
                flat = flat.astype(want)
            zq = int(_as_object(_static_quantize_padding_asymmetric(flat, 1.0, q.element_bits, device=q._device, as_object=False,
                                                                     rng=rng)).reshape(-1)[0])
            ct.buf.upload_at(n * eng.limbs * 8, np.array([zq & (2 ** 64 - 1), zq >> 64][:eng.limbs], dtype=np.uint64))
            del weights._weights["zzz"]
        for k in order:
            del weights._weights[k]
        self.shape_dict = shape_dict
        if order:
            weights._weights[order[0]] = ct.mark_ready() if device else ct.to_host()
        weights.walking_order = sorted(weights._weights.keys(), key=str)
        return weights

    def _back_degrees(self, degree, total_degree):
        """decrypt_unquantize's (degree, total_degree) after their checks, before anything is touched: both None = no scaling; degree
        defaults to the one the last quantize_encrypt took; ValueError for a value _check_degree refuses, a total_degree without any
        degree, a degree given without a total_degree."""
        _check_degree(degree, "degree")
        _check_degree(total_degree, "total_degree")
        if total_degree is None:
            if degree is not None:
                raise ValueError("degree without total_degree: the back end divides by total_degree / degree first (jzf_aggregator.py:902)")
            return None, None
        if degree is None:
            degree = self.degree
        if degree is None:
            raise ValueError("total_degree without a degree: pass degree= (no quantize_encrypt of this client took one)")
        return degree, total_degree

    def _host_tail(self, weights, unnormalize, degree, total_degree, last):
        """Client.get_aggregated_model behind the unquantise (jzf_aggregator.py:902-907) with the reference's NumPy operations on host
        layers: `/= (degrees / self.degree)`, unnormalize (which records np.mean / np.std of the divided values), `/= self.degree`,
        `+ weights_last_round` -- each only when asked (the reference's dense job would raise at :907 with its weights_last_round None)."""
        w = weights._weights
        if total_degree is not None:
            s = total_degree / degree
            for k in weights.walking_order:
                w[k] = w[k] / s
        if unnormalize:
            weights = self.unnormalize(weights)
            w = weights._weights
        if total_degree is not None:
            for k in weights.walking_order:
                w[k] = w[k] / degree
        if last is not None:
            for k in weights.walking_order:
                w[k] = np.asarray(last[k]) + w[k]
        return weights

    def decrypt_unquantize(self, weights, out=None, unnormalize=False, degree=None, total_degree=None, last_round=None):
        """degree, total_degree, last_round (new): Client.get_aggregated_model's steps around unnormalize (jzf_aggregator.py:902-907), in
        its order and with its operations: `/ (total_degree / degree)` (total_degree = the arbiter's sum of the clients' degrees, :380;
        the quotient is computed once in Python), [unnormalize: `+ mean`, np.mean / np.std of THAT value recorded], `/ degree`,
        `last_round + w` -- two correctly rounded divisions and no fused multiply-add.  degree defaults to the one the last
        quantize_encrypt took; both None: no scaling.  last_round (None: no add): a Weights / dict of host arrays; with out=, of framework
        device tensors of the layers' shapes (any of the four dtypes, upcast exactly), where last_round[name] may be out[name] itself --
        the model is then updated in place.  With out= all of it is the ONE store + statistics pass (flashe_finish_layers_dev).
        ValueError before anything is touched: a degree or total_degree that is zero, negative, non-finite or not a real number, a
        total_degree without a degree, a degree without a total_degree.

        out (new): {layer name: framework float device tensor (float64 / float32 / float16 / bfloat16) of the layer's shape} -- the
        values are written there in place (see _decrypt_unquantize_tensors) and weights._weights[name] becomes out[name].  unnormalize
        (new): QuantizingClient.unnormalize after it (jzf_quantize.py:549-564): the layer mean added back and the statistics of the next
        round's alpha refreshed -- with `out`, on the device, bit-identical to np.mean / np.std of the float64 result.

        What Client.aggregate does between "begin decryption" and "end decoding" (jzf_aggregator.py:881-899): `weights.decrypted(self)`
        (jzf_weights.py:334-335 -> _Client.decrypt) of the ONE flattened aggregate, `unflatten_weights` by `self.shape_dict`, then
        QuantizingClient.unquantize layer by layer (jzf_quantize.py:493-540) -- as ONE launch (flashe_decrypt_unquantize_model_dev): the
        aggregate -- a DeviceVector, uint64 limbs or object ints -- is decrypted with the prefixes `set_idx_list` left behind and comes
        back as unquantised float64 layers.  The SPARSE job (location lists in `cipher.masks`; it sets `self.shape_dict =
        shape_dict_used_for_sparsification` first, :893-894) decrypts on the device with the sparse minus-mask pass and unquantises the
        dense result in a second launch (flashe_unquantize_model_dev).  PRECOMPUTED decrypt masks (the handles prepare_decrypt leaves) are
        added by the same one launch in place of the PRF streams (flashe_decrypt_prepared_unquantize_model_dev / _unbatch_: the batched job's
        decrypt + unbatch becomes one launch); the prefixes set_idx_list leaves uncovered (dropouts) go through a PRF launch first.  The
        cache is consumed as the call-by-call decrypt consumes it; the encrypt cache of the next round is not touched.  Masks a caller
        assigned as plain arrays take the same sequence call by call."""
        q, c = self.quantizer, self.cipher
        degree, total_degree = self._back_degrees(degree, total_degree)
        if out is not None:
            return self._decrypt_unquantize_tensors(weights, out, unnormalize, degree, total_degree, last_round)
        if unnormalize or total_degree is not None or last_round is not None:
            last = None
            if last_round is not None:
                last = _layers_of(last_round)
                bad = [k for k in (self.shape_dict or {}) if k not in last or interop.is_foreign(last[k])]
                if bad:
                    raise TypeError(f"last_round: without out= it holds a host array for every layer, not so for {bad}")
            return self._host_tail(self.decrypt_unquantize(weights), unnormalize, degree, total_degree, last)
        fus = self.fuse and c.masks is None and c.prp_seed is not None and hasattr(c.engine, "decrypt_unquantize_model_dev")
        mode = None
        if fus:
            c._reconcile_prepared()
            mode = self._prepared_mode(c.next_iter_decrypt_prepared)
            fus = mode is not False
        k0 = weights.walking_order[0]
        from .cipher import _SparseMinus
        prep = c.next_iter_decrypt_prepared
        sparse_dev = (self.fuse and c.masks is not None and c.masking_scheme == "single" and not self.batch and c.prp_seed is not None
                      and set(prep) == {"minus"} and isinstance(prep["minus"], _SparseMinus) and hasattr(c.engine, "unquantize_model_dev"))
        if sparse_dev:
            keep = []                                 # (the minus-mask pass's result: alive until the download has synchronised)
            dout, n = self._sparse_floats(weights._weights[k0], [_size(shape) for shape in self.shape_dict.values()], keep)
            weights._weights[k0] = dout.download(np.float64, n)
            return self.unflatten_weights(weights)
        if not fus:
            res = self.cipher.decrypt(weights._weights[k0], device=False)
            if isinstance(res, np.ndarray) and res.dtype == np.uint64 and res.ndim == 2:
                from .cipher import _from_limbs
                res = _from_limbs(res, "object")          # (limbs in, limbs out: the layer-by-layer sequence works on the reference's object ints)
            weights._weights[k0] = res
            return self.unquantize(self.unflatten_weights(weights))
        add_idx, minus_idx = self._decrypt_prefixes(mode)
        dv = self._wide_aggregate(weights._weights[k0])
        n = len(dv)
        if self.batch:
            names = list(self.shape_dict)
            sizes = [_size(shape) for shape in q.shape_list]
            out = self._decrypt_floats(dv, sizes, mode, add_idx, minus_idx).download(np.float64, sum(sizes))
            del weights._weights[k0]
            at = 0
            for name, shape, s_ in zip(names, q.shape_list, sizes):
                weights._weights[name] = out[at:at + s_].reshape(shape)
                at += s_
            weights.walking_order = sorted(weights._weights.keys(), key=str)
            return weights
        sizes = [_size(shape) for shape in self.shape_dict.values()]
        weights._weights[k0] = self._decrypt_floats(dv, sizes, mode, add_idx, minus_idx).download(np.float64, n)
        return self.unflatten_weights(weights)

    def _decrypt_prefixes(self, mode):
        """The prefix lists set_idx_list left behind: those of the online decrypt, or -- mode "ctx" -- the extras the prepared masks do
        not cover (dropouts; empty when nobody dropped out)."""
        c = self.cipher
        if c.masking_scheme != "double":
            return [], [c._idx_of(p) for p in c.index_prefix_for_minus]
        add_idx = [c._idx_of(p) for p in (c.index_prefix_for_add or [])]
        minus_idx = [c._idx_of(p) for p in (c.index_prefix_for_minus or [])]
        if not add_idx and not minus_idx and mode != "ctx":
            raise KeyError('add')
        return add_idx, minus_idx

    def _wide_aggregate(self, v, keep=None):
        """The flattened aggregate -- a DeviceVector, uint64 limbs, object ints or, with `keep` (out=), a framework integer tensor, read
        in place and its owner appended to keep -- as a DeviceVector of L limbs in HBM (a compact uint32 aggregate widened: the fused
        launches read one-limb vectors)."""
        from .engine import DeviceVector
        c = self.cipher
        if keep is not None and interop.is_foreign(v):
            v, kv = c._foreign_vec(c.engine, v, "aggregate")
            keep.append(kv)
        elif not isinstance(v, DeviceVector):
            v = np.asarray(v)
            if v.dtype == object:
                v = v.reshape(-1)
        dv, _kind = c._on_device(v, full_width=True)
        return c._as_wide(dv)

    def _back_table(self, sizes, n):
        """The back end's layer table over an aggregate of n elements: (start, None, alpha, False) per layer of `sizes`, the last layer
        running to the end."""
        q = self.quantizer
        if sum(sizes) > n:
            raise ValueError(f"the aggregate has {n} elements, shape_dict describes {sum(sizes)}")
        table, at = [], 0
        for li, size in enumerate(sizes):
            table.append((at, None, q.alpha_list[li], False))
            at += size
        return table

    def _batched_back_table(self, sizes, n):
        """The same for a batched aggregate of n elements: ((size, None, alpha, False) per layer, field_bits), every layer padded to whole
        elements on its own."""
        q = self.quantizer
        field_bits = _field_bits(q.element_bits, q.num_clients)
        bs = self.int_bits // field_bits
        if sum((s_ + bs - 1) // bs for s_ in sizes) != n:
            raise ValueError(f"the aggregate has {n} elements, the batched layers describe {sum((s_ + bs - 1) // bs for s_ in sizes)}")
        return [(s_, None, q.alpha_list[li], False) for li, s_ in enumerate(sizes)], field_bits

    def _sparse_floats(self, v, sizes, keep):
        """The sparse job's back end: the minus-mask pass over the aggregate v (result in HBM, appended to keep), then the unquantise of
        the dense model in a second launch.  Returns (the n float64 values as a device buffer, n)."""
        q, c = self.quantizer, self.cipher
        eng = c.engine
        dec = c._as_wide(c.decrypt(v, device=True))
        n = len(dec)
        table = self._back_table(sizes, n)
        dout = eng.alloc(max(8 * n, 16))
        if n:
            dec.wait_on(eng)
            eng.unquantize_model_dev(n, 0, n, dec.buf, table, q.element_bits, q.num_clients, dout)
        keep.append(dec)
        return dout, n

    def _decrypt_floats(self, dv, sizes, mode, add_idx, minus_idx):
        """The fused back end of the flattened aggregate `dv` (in HBM, L limbs): the model's float64 values in walking order as a device
        buffer -- batched: the sum(sizes) values of the layers (unbatch + `[:size]` + unquantise in one launch behind the decrypt); else
        all n elements, the last layer running to the end (decrypt + unquantise in one launch).  mode "ctx": with the ctx's prepared
        decrypt masks, the prefix lists being the extras, in ONE launch either way (two with extras); the cache is consumed."""
        from . import cipher as _cipher_mod
        q, c = self.quantizer, self.cipher
        eng, n = c.engine, len(dv)
        if mode == "ctx":
            c._check_prepared_len(c.next_iter_decrypt_prepared['add'], n)          # (the call-by-call decrypt's error; the cache stays)
        if self.batch:
            layers, field_bits = self._batched_back_table(sizes, n)
            dout = eng.alloc(max(8 * sum(sizes), 16))
            if mode == "ctx":
                eng.decrypt_prepared_unbatch_unquantize_model_dev(c.iter_index, add_idx, minus_idx, _cipher_mod.N_JOBS, layers, q.element_bits, field_bits,
                                                                  q.num_clients, dv.buf, n, dout)
            else:
                dec = eng.alloc_vec(max(n, 1))
                if n:
                    eng.decrypt_dev(c.iter_index, add_idx, minus_idx, n, _cipher_mod.N_JOBS, dv.buf, dec)
                eng.unbatch_unquantize_model_dev(layers, q.element_bits, field_bits, q.num_clients, dec, n, dout)
            self._decrypt_done(mode)
            return dout
        table = self._back_table(sizes, n)
        dout = eng.alloc(max(8 * n, 16))
        if mode == "ctx":
            eng.decrypt_prepared_unquantize_model_dev(c.iter_index, add_idx, minus_idx, n, _cipher_mod.N_JOBS, dv.buf, table, q.element_bits,
                                                      q.num_clients, dout)
        elif n:
            eng.decrypt_unquantize_model_dev(c.iter_index, add_idx, minus_idx, n, _cipher_mod.N_JOBS, 0, n, dv.buf, table, q.element_bits,
                                             q.num_clients, dout)
        self._decrypt_done(mode)
        return dout

    # ---- a framework's device tensors either side of the client step (new; interop.py) ---------------------------------------
    def _quantize_encrypt_tensors(self, weights, device, normalize, rng=None, degree=None):
        """quantize_encrypt with framework device tensors among the layers: each foreign layer is read in place (its own dtype; a layer
        that needs a conversion -- 16-bit, float32 quantised in float64, or normalised -- goes through one streaming pass into engine
        scratch, flashe_quantize_encrypt_tensors_dev / flashe_quantize_batch_tensors_dev), host layers go up as in the host path.  Bit for
        bit the host path on `t.cpu().numpy()` (float16 / bfloat16: `t.float().cpu().numpy()`), with `normalize()` first when asked.
        The refusals, then the front end for tensors: 6-field rows (start, pointer, alpha, shift, dtype code, flags) for the *_tensors_dev
        entry points, and _encrypt_tail behind them.  degree: host layers are multiplied on the host, and ONE stage pass of the caller's
        (_stage_scaled) multiplies and normalises the tensors into engine scratch, which the same entry points then read as plain float32 /
        float64 layers without a shift."""
        q, c = self.quantizer, self.cipher
        if degree is not None and not hasattr(c.engine, "stage_layers_dev"):
            raise TypeError("degree with framework tensors needs an engine with flashe_stage_layers_dev")
        zzz = None
        if "zzz" in weights._weights:                 # the sparse job: compact layers (Sparsifier's CompactLayer or any tensors) + 'zzz'
            if not self.fuse:
                raise TypeError("framework tensors in the sparse job need the fused client step (fuse=True)")
            if self.batch:
                raise TypeError("framework tensors are not supported by batched sparse jobs")
            if c.prp_seed is not None:
                c._reconcile_prepared()
            if c.next_iter_encrypt_prepared:
                raise TypeError("framework tensors are not supported by sparse jobs with precomputed encrypt masks")
            if not self._fusable(weights):
                raise TypeError("framework tensors in the sparse job need the one-value 'zzz' layer at the end of the walking order")
            zzz = weights._weights["zzz"]
            if interop.is_foreign(zzz):
                raise TypeError("the sparse job's 'zzz' layer must be a host value")
            zzz = np.asarray(zzz)
        elif not self._fusable(weights):
            raise TypeError("framework tensors need the fused client step (fuse=True, no location masks, precomputed encrypt masks only as "
                            "the handles prepare_encrypt leaves)")
        eng = c.engine
        mode = self._prepared_mode(c.next_iter_encrypt_prepared) if zzz is None else None
        order = list(weights.walking_order)
        if zzz is not None:
            order = order[:-1]
        scaled = lambda v: v if degree is None or interop.is_foreign(v) else np.asarray(v) * degree
        layers = [_layer_source(eng, scaled(weights._weights[k]), f"layer {k!r}") for k in order]
        sizes = [size for _x, _code, _hdt, size, _shape in layers]
        alphas = _round_alphas(q, sizes + ([int(zzz.size)] if zzz is not None else []))      # (set_layer_size_list on the sizes the tensors report)
        q.r_max_list, q.alpha_list = [], []
        c.set_idx_list(mode="encrypt")
        ptrs, keep = _stage_host_layers(eng, [x for x, _code, _hdt, _size, _shape in layers])
        owners = [x.keep for x, _code, _hdt, _size, _shape in layers if not isinstance(x, np.ndarray)]
        staged = None
        if degree is not None:
            staged, scratch = _stage_scaled(eng, [(ptrs[li], code, hdt, size, None if isinstance(x, np.ndarray) else degree, alphas[li],
                                                   q.past_layer_mean_list[li] if normalize else None)
                                                  for li, (x, code, hdt, size, _shape) in enumerate(layers)])
            keep.append(scratch)
        rows, starts, n = [], [], 0
        for li, (_x, code, hdt, size, _shape) in enumerate(layers):
            alpha = alphas[li]
            q.r_max_list.append(alpha * q.num_clients)
            q.alpha_list.append(alpha)
            if staged is not None:
                rows.append((n, staged[li][0], alpha, 0.0, staged[li][1], 0))
            else:
                shift, flags = _tensor_flags(hdt, alpha, normalize, q.past_layer_mean_list[li])
                rows.append((n, ptrs[li], alpha, shift, code, flags))
            starts.append(n)
            n += size
        launch = (eng.quantize_encrypt_tensors_dev, eng.quantize_encrypt_prepared_tensors_dev,                # (the batched two also take n)
                  lambda r, *a: eng.quantize_batch_tensors_dev(r, n, *a),
                  lambda r, *a: eng.quantize_batch_encrypt_prepared_tensors_dev(r, n, *a))
        shape_dict = {k: layer[4] for k, layer in zip(order, layers)}
        return self._encrypt_tail(weights, device, mode, order, zzz, sizes, starts, shape_dict, rows, launch, keep, hold=owners, normalize=normalize,
                                  rng=rng)

    def _decrypt_unquantize_tensors(self, weights, out, unnormalize, degree=None, total_degree=None, last_round=None):
        """decrypt_unquantize into the caller's tensors: the fused back end writes the flat float64 model into engine scratch, one
        streaming pass (flashe_store_layers_dev) adds the layer means back (unnormalize) and stores every layer in its tensor's dtype --
        float64 -> float32 -> 16 bits, each step round to nearest even -- and, with unnormalize, sums every layer the way np.mean /
        np.std do, so past_layer_mean_list / past_layer_std_list get the host path's np.float64 values.  Only those 16 bytes per layer come
        back to the host.  Own-stream engines synchronise before returning.  With total_degree / degree / last_round the pass is
        flashe_finish_layers_dev: the two divisions and the add ride it, the statistics are those of the divided, shifted values."""
        from .cipher import _SparseMinus
        q, c = self.quantizer, self.cipher
        scaling = total_degree is not None or last_round is not None
        if scaling and not hasattr(c.engine, "finish_layers_dev"):
            raise TypeError("degree / last_round with out= need an engine with flashe_finish_layers_dev")
        if "zzz" in weights._weights:
            raise TypeError("out= takes the dense aggregate, not an upload with the sparse job's 'zzz' layer")
        sparse = c.masks is not None
        mode = False
        if sparse:                                    # the sparse job: location masks, the single-mask minus pass (decrypt_unquantize)
            if not self.fuse:
                raise TypeError("out= in the sparse job needs the fused client step (fuse=True)")
            if self.batch:
                raise TypeError("out= is not supported by batched sparse jobs")
            if c.masking_scheme != "single":
                raise TypeError("out= is not supported with the sparse job's dense-position double mask (masking_scheme 'double')")
            prep = c.next_iter_decrypt_prepared
            if c.prp_seed is None or set(prep) != {"minus"} or not isinstance(prep["minus"], _SparseMinus):
                raise TypeError("out= in the sparse job needs the location masks set_idx_list(mode='decrypt') leaves (no precomputed decrypt "
                                "masks)")
            mode = None
        elif self.fuse and c.prp_seed is not None:
            c._reconcile_prepared()
            mode = self._prepared_mode(c.next_iter_decrypt_prepared)
        if mode is False:
            raise TypeError("out= needs the fused client step (fuse=True, precomputed decrypt masks only as the handles prepare_decrypt leaves)")
        if self.shape_dict is None:
            raise ValueError("decrypt_unquantize(out=...) needs the layer shapes a quantize_encrypt left behind (shape_dict)")
        eng = c.engine
        names = list(self.shape_dict)
        shapes = list(q.shape_list) if self.batch else [self.shape_dict[k] for k in names]
        missing = [k for k in names if k not in out]
        if missing:
            raise KeyError(f"out has no tensor for layer(s) {missing}")
        fas = []
        for k, shape in zip(names, shapes):
            if not interop.is_foreign(out[k]):
                raise TypeError(f"out[{k!r}]: expected a framework device tensor, got {type(out[k]).__name__}")
            fa = eng.foreign(out[k], writable=True, what=f"out[{k!r}]")
            if fa.dtype not in _TENSOR_CODES:
                raise TypeError(f"out[{k!r}]: unsupported dtype {fa.dtype} (float64, float32, float16 or bfloat16)")
            if tuple(fa.shape) != tuple(shape):
                raise ValueError(f"out[{k!r}]: expected shape {tuple(shape)}, got {tuple(fa.shape)}")
            fas.append(fa)
        lasts = None
        if last_round is not None:
            last, lasts = _layers_of(last_round), []
            for k, shape, fa in zip(names, shapes, fas):
                if k not in last or not interop.is_foreign(last[k]):
                    raise TypeError(f"last_round[{k!r}]: with out= expected a framework device tensor")
                la = fa if last[k] is out[k] else eng.foreign(last[k], what=f"last_round[{k!r}]")
                if la.dtype not in _TENSOR_CODES:
                    raise TypeError(f"last_round[{k!r}]: unsupported dtype {la.dtype} (float64, float32, float16 or bfloat16)")
                if tuple(la.shape) != tuple(shape):
                    raise ValueError(f"last_round[{k!r}]: expected shape {tuple(shape)}, got {tuple(la.shape)}")
                lasts.append(la)
        k0 = weights.walking_order[0]
        v = weights._weights[k0]
        keep = [fa.keep for fa in fas] + [la.keep for la in (lasts or [])]
        sizes = [_size(shape) for shape in shapes]
        tail = (degree, total_degree, lasts) if scaling else None
        if sparse:
            dout, _n = self._sparse_floats(v, sizes, keep)
            return self._store_tensors(weights, out, names, fas, sizes, dout, keep, unnormalize, tail)
        add_idx, minus_idx = self._decrypt_prefixes(mode)
        dout = self._decrypt_floats(self._wide_aggregate(v, keep), sizes, mode, add_idx, minus_idx)
        return self._store_tensors(weights, out, names, fas, sizes, dout, keep, unnormalize, tail)

    def _store_tensors(self, weights, out, names, fas, sizes, dout, keep, unnormalize, tail=None):
        """The back end's flat float64 model `dout` (in HBM) into the out= tensors, with the exact statistics when unnormalising.  tail =
        (degree, total_degree, last-round ForeignArrays or None): jzf_aggregator.py:902-907 in the same pass (flashe_finish_layers_dev)."""
        q, eng = self.quantizer, self.cipher.engine
        n_values = sum(sizes)
        layers, at = [], 0
        if tail is not None:
            degree, total_degree, lasts = tail
            scaled = total_degree is not None
            s = float(total_degree / degree) if scaled else 1.0            # (:902: the quotient once, in Python)
            flags = ((_lib.FINISH_DIV_TOTAL | _lib.FINISH_DIV_OWN) if scaled else 0) | (_lib.FINISH_SHIFT if unnormalize else 0) | \
                    (_lib.FINISH_ADD_LAST if lasts is not None else 0)
        for li, (fa, size) in enumerate(zip(fas, sizes)):
            shift = float(q.past_layer_mean_list[li]) if unnormalize else 0.0
            if tail is not None:
                la = lasts[li] if lasts is not None else None
                layers.append((at, fa.ptr, la.ptr if la is not None else None, s, shift, float(degree) if scaled else 1.0, _TENSOR_CODES[fa.dtype],
                               _TENSOR_CODES[la.dtype] if la is not None else 0, flags))
            else:
                layers.append((at, fa.ptr, 1.0, shift, _TENSOR_CODES[fa.dtype], _lib.TENSOR_SHIFT if unnormalize else 0))
            at += size
        stats = eng.alloc(max(16 * len(layers), 16)) if unnormalize else None
        if n_values and tail is not None:
            eng.finish_layers_dev(dout, n_values, layers, block=np.getbufsize() if unnormalize else 0, stats=stats)
        elif n_values:
            eng.store_layers_dev(dout, n_values, layers, block=np.getbufsize() if unnormalize else 0, stats=stats)
        eng.hold(keep + [dout])
        if unnormalize:
            st = stats.download(np.float64, 2 * len(layers))          # (synchronises: 16 bytes per layer)
            for li, size in enumerate(sizes):
                if size:
                    # np.mean = S / n, np.std = sqrt(S2 / n): the same float64 operations on NumPy's own sums
                    q.past_layer_mean_list[li] = np.float64(st[2 * li]) / size
                    q.past_layer_std_list[li] = np.sqrt(np.float64(st[2 * li + 1]) / size)
                else:
                    e = np.zeros(0, dtype=np.float64)
                    q.past_layer_mean_list[li], q.past_layer_std_list[li] = np.mean(e), np.std(e)
        elif not eng.shared_stream:
            eng.sync()
        for k in list(weights._weights):
            del weights._weights[k]
        for k in names:
            weights._weights[k] = out[k]
        weights.walking_order = sorted(weights._weights.keys(), key=str)
        return weights

    def prepare_encrypt(self):
        if self.precompute:
            self.cipher.prepare_encrypt()

    def prepare_decrypt(self):
        if self.precompute:
            self.cipher.prepare_decrypt()


# ---- a cohort of consecutive clients hosted on one GPU (new) --------------------------------------------------------------------
COHORT_CHAIN, STAGED_CHAIN, PER_CLIENT = "cohort-chain", "staged-chain", "per-client"
PREPARED_COHORT, PREPARED_STAGED = "prepared-cohort", "prepared-staged"   # with the cohort's own mask cache (FlasheCohort.prepare_encrypt)
CUT_CHAIN = "cut-chain"          # a short cohort's summed chain cut into runs of clients + one combine pass (FlasheCohort(cut=True))
_COHORT_MAX_LINKS = 128          # outputs of one chained launch (kMaxLinks, kernels.hip)
_COHORT_MAX_STREAMS = 144        # PRF streams of one chained launch (kCohortMaxStreams, cohort_streams.h): present clients + runs


class _Layers(object):
    """The surface FlasheClient walks (JZFOrderDictWeights': walking_order, _weights) around a dict of layers."""

    def __init__(self, layers):
        self._weights = dict(layers)
        self.walking_order = sorted(self._weights.keys(), key=str)


class CohortPlan(object):
    """What plan_cohort returns: names / shapes / sizes / starts of the shared layer table, n (values of one model), n_elems (ciphertext
    elements of one upload: n, or the batched count), draw_offsets (the p-th present client's first draw in the client-major draws), path
    and the reason for it, present (the local positions of the clients that report: all of them unless some dropped out) and runs (the
    runs of consecutive positions among them); parts: the runs of clients a "cut-chain" launch is cut into (1 on every other path)."""

    def __init__(self, names, shapes, sizes, starts, n, n_elems, draw_offsets, path, reason, present=None, runs=1, parts=1):
        self.names, self.shapes, self.sizes, self.starts = names, shapes, sizes, starts
        self.n, self.n_elems, self.draw_offsets, self.path, self.reason = n, n_elems, draw_offsets, path, reason
        self.present, self.runs, self.parts = list(range(len(draw_offsets))) if present is None else list(present), runs, parts


class CohortUpload(object):
    """FlasheCohort.quantize_encrypt's result: ciphertexts (one DeviceVector per present client), partial_sum (their sum mod 2^b), path
    and present (the GLOBAL cipher indices of the clients the upload holds, ascending: what a decrypt of the sum passes to
    set_idx_list), and draws: "inline" when the launch that consumed the stochastic-rounding draws generated them itself (a prepared
    un-batched cohort over Philox generators), "buffer" when they were materialised in HBM first."""

    def __init__(self, ciphertexts, partial_sum, path, present=None, draws="buffer"):
        self.ciphertexts, self.partial_sum, self.path, self.present, self.draws = ciphertexts, partial_sum, path, present, draws


def _present_runs(present, count):
    """The refusals of a `present` list (one local position per Weights, strictly ascending, none negative) and the runs of consecutive
    positions it forms.  present=None: everyone, one run."""
    if present is None:
        return list(range(count)), 1
    try:
        pos = [int(p) for p in present]
        exact = all(p == q for p, q in zip(pos, present))
    except (TypeError, ValueError):
        raise ValueError("present: a list of the local positions of the clients that report") from None
    if not exact:
        raise ValueError("present: the positions must be integers")
    if len(pos) != count:
        raise ValueError(f"present names {len(pos)} clients, got {count} Weights")
    if any(p < 0 for p in pos):
        raise ValueError("present: a negative position")
    if any(b <= a for a, b in zip(pos, pos[1:])):
        raise ValueError("present: the positions must be strictly ascending (sorted, no client twice)")
    return pos, 1 + sum(1 for a, b in zip(pos, pos[1:]) if b != a + 1)


def _telescoped(idxs):
    """(add, minus) of engine.telescope for strictly ascending indices: one past every run's end, every run's start, ascending."""
    add, minus = [], []
    for i in idxs:
        if add and add[-1] == i:
            add[-1] = i + 1
        else:
            add.append(i + 1)
            minus.append(i)
    return add, minus


def _layer_shape(v):
    return tuple(int(d) for d in (v.shape if hasattr(v, "shape") else np.shape(v)))


def _layer_is_f64(v):
    """Does the layer compute in float64 whatever its alpha is -- a float64 array, or a host array that is not a float array at all?"""
    name = str(getattr(v, "dtype", "float64")).replace("torch.", "")
    if isinstance(v, np.ndarray) or not hasattr(v, "shape"):
        return name != "float32"                   # (a host layer that is not float32 is quantised as float64)
    return name not in ("float32", "float16", "bfloat16")


def _one_model(clients):
    """(names, shapes, f64, mixed) of the ONE model that the clients' (walking order, layers) pairs describe: ValueError naming the client and
    the layer where the names, their order or a shape differ from client 0's; mixed: a layer is float64 for some clients only."""
    names, shapes, f64, mixed = None, [], [], False
    for c, (order, layers) in enumerate(clients):
        if names is None:
            names = order
            shapes = [_layer_shape(layers[k]) for k in order]
            f64 = [_layer_is_f64(layers[k]) for k in order]
            continue
        if order != names:
            odd = next((k for k in order if k not in names), None) or next((k for k in names if k not in order), None)
            if odd is None:
                odd = next(a for a, b in zip(order, names) if a != b)
                raise ValueError(f"client {c}: layer {odd!r} comes at another place of the walking order than in client 0's")
            raise ValueError(f"client {c}: layer {odd!r} is not a layer of every client of the cohort")
        for li, k in enumerate(order):
            shp = _layer_shape(layers[k])
            if shp != shapes[li]:
                raise ValueError(f"client {c}: layer {k!r} has shape {shp}, client 0's has {shapes[li]}")
            mixed |= _layer_is_f64(layers[k]) != f64[li]
    return names, shapes, f64, mixed


def cohort_admission_length(cu_count):
    """The shortest vector the summed chain takes uncut: two whole 256-element tiles for each of the chip's 16 x cu_count waves."""
    return (2 * 16 * int(cu_count) - 1) * 256 + 1


_COHORT_BATCH_SIZES = (5, 6, 7)                     # the values per element compiled into the batched cohort chain (prf_chain_cohort_batch_kernel)
# the widths compiled into the compact chains, dense and sparse (FLASHE_FIXED32_WIDTHS, csrc/kernels.hip)
_COMPACT_COHORT_WIDTHS = (16, 20, 23, 24, 32)


def compact_cohort_blocks(n, int_bits, n_jobs):
    """The AES blocks of an n-element vector at int_bits <= 64: every one of the n_jobs chunks (n % n_jobs of them one element longer) is
    cut into blocks of m = 128 // int_bits elements of its own."""
    m, (d, r) = 128 // int(int_bits), divmod(int(n), int(n_jobs))
    return r * ((d + m) // m) + (int(n_jobs) - r) * ((d + m - 1) // m)


def compact_cohort_admission_length(cu_count, int_bits, n_jobs):
    """The shortest vector the summed compact chain takes uncut: 2 x 128 AES blocks for each of the chip's 16 x cu_count waves."""
    need = 2 * 128 * 16 * int(cu_count)
    lo, hi = 1, need * (128 // int(int_bits))           # (hi: need whole blocks in one chunk at the least)
    while lo < hi:
        mid = (lo + hi) // 2
        if compact_cohort_blocks(mid, int_bits, n_jobs) >= need:
            hi = mid
        else:
            lo = mid + 1
    return lo


_CUT_MAX_PARTS, _CUT_MIN_OUTPUTS = 16, 4           # kCutMaxParts, kCutMinOutputs (csrc/cohort_cut.h)


def cohort_cut_items(n, int_bits, n_jobs, compact=False, n_elems=None):
    """The items of one uncut chain over an n-element vector (csrc/cohort_cut.h): half tiles of 128 elements in the wide layout, tiles of
    128 AES blocks in the compact one -- two AES blocks per lane and stream either way.  n_elems (a BATCHED job, wide layout): the chain
    runs over the model's batched elements, 2 * ceil(n_elems / 256) half tiles."""
    if compact:
        return (compact_cohort_blocks(n, int_bits, n_jobs) + 127) // 128
    return 2 * ((int(n if n_elems is None else n_elems) + 255) // 256)


def cohort_cut_parts(n_clients, items, cu_count):
    """The mirror of cohort_cut_parts in csrc/cohort_cut.h (tests/test_cohort_cut_host.py holds the two against each other): the runs of
    consecutive clients the cut launch makes of a cohort whose uncut chain has `items` items -- as many as fill the chip once (the
    largest count whose items do not outnumber the chip's 16 x cu_count waves), never fewer than four clients per piece, at most 16
    pieces; one piece from half an item per wave upward.
    0: not a shape of the cut launch.  Piece p holds clients [C p // parts, C (p + 1) // parts)."""
    C, items, cus = int(n_clients), int(items), int(cu_count)
    if C < 1 or C > _COHORT_MAX_LINKS or items < 1 or cus < 1:
        return 0
    return max(1, min(16 * cus // items, max(1, C // _CUT_MIN_OUTPUTS), _CUT_MAX_PARTS))


def cohort_cut_pieces(idxs, items, cu_count):
    """The mirror of cohort_cut_pieces in csrc/cohort_cut.h (tests/test_cohort_cut_pieces_host.py holds the two against each other): the
    pieces of a cohort given by ANY strictly ascending cipher indices -- every gap is a cut the round imposes.  Every run of consecutive
    indices starts as one piece; while the pieces number fewer than max(runs, cohort_cut_parts(...)) the run with the most clients per
    piece takes one more (the lower run on a tie), as long as its pieces keep four clients; inside a run the pieces are even.
    Returns begins: the position in idxs of every piece's first client and len(idxs) at the end (len(begins) - 1 pieces); [] where the
    cut launch declines -- cohort_cut_parts' cases, more than 16 runs, indices that are not strictly ascending or hold 2^32 - 1."""
    idxs = [int(i) for i in idxs]
    C = len(idxs)
    rule = cohort_cut_parts(C, items, cu_count)
    if not rule or any(i < 0 or i >= 2 ** 32 - 1 for i in idxs) or any(b <= a for a, b in zip(idxs, idxs[1:])):
        return []
    start = [0] + [v for v in range(1, C) if idxs[v] != idxs[v - 1] + 1] + [C]
    runs = len(start) - 1
    if runs > _CUT_MAX_PARTS:
        return []
    lens, k = [start[r + 1] - start[r] for r in range(runs)], [1] * runs
    for _ in range(runs, max(rule, runs)):
        best = -1
        for r in range(runs):
            if lens[r] // (k[r] + 1) >= _CUT_MIN_OUTPUTS and (best < 0 or lens[r] * k[best] > lens[best] * k[r]):
                best = r
        if best < 0:
            break
        k[best] += 1
    return [start[r] + lens[r] * q // k[r] for r in range(runs) for q in range(k[r])] + [C]


def plan_cohort(weights_list, int_bits, cu_count, element_bits=16, batch=False, mask="double", num_clients=None, precompute=False, chain=True,
                location_masks=False, compact=False, n_jobs=None, cohort_masks=False, present=None, compact_runs=False, cut=False, cut_any=False,
                one_limb=False, limb_runs=False):
    """The engine-free part of FlasheCohort.quantize_encrypt: checks that the clients' Weights describe one model (the same layer names
    in the same walking order with the same shapes: ValueError naming the client and the layer otherwise; a sparse upload -- a 'zzz'
    layer or location masks -- is a TypeError), lays out the shared layer table and the client-major draws, and picks the path:
      "cohort-chain"  one chained launch from the floats (flashe_quantize_encrypt_cohort_dev): double mask, int_bits > 64, not batched, at
                      most 128 clients, a model of at least cohort_admission_length(cu_count) values, FLASHE_CHAIN not 0, every layer
                      float64 for all clients or for none.  A batched job at int_bits > 64 takes it too
                      (flashe_quantize_batch_encrypt_cohort_dev) when bs = int_bits // (element_bits + ceil(log2 num_clients)) is 5, 6
                      or 7 -- what element_bits 16 gives at int_bits 120 / 128 -- with the length rule counted in batched elements
                      (n_elems, every layer padded to whole elements on its own);
      "per-client"    precompute handles (and masks other than single / double): the clients' own steps, then aggregate;
      "staged-chain"  everything else: a quantise (+ batch) pass per client into plaintexts, then the summed batch encrypt.
    compact=True (FlasheCohort(compact=True): uint32 ciphertexts at int_bits <= 32) chains through
    flashe_quantize_encrypt_cohort_u32_dev instead: int_bits 16 / 20 / 23 / 24 / 32 in place of int_bits > 64, and a model of at least
    compact_cohort_admission_length(cu_count, int_bits, n_jobs) values (n_jobs: the chunking of the counters, default cipher.N_JOBS)
    and fewer than 2^32 in place of the length rule above; the other conditions and every fallback are the same.
    cohort_masks=True (the cohort holds the masks of FlasheCohort.prepare_encrypt: a precompute job under the double mask) answers
      "prepared-cohort"  one online launch from the floats and the masks, no AES (flashe_quantize_combine_cohort_dev, its _u32 form with
                         compact=True, flashe_quantize_batch_combine_cohort_dev for a batched job): any int_bits, any length, any number
                         of clients.  The draws are laid out client-major for a buffer in HBM (draw_offsets); an un-batched round
                         whose rng= generators are over np.random.Philox materialises none -- the launch generates them at those
                         positions (flashe_quantize_combine_cohort_philox_dev / _u32_dev, FlasheCohort.quantize_encrypt);
      "prepared-staged"  a layer that is float64 for some clients only (no shared row), or a batched job in the compact layout: a
                         quantise (+ batch) pass per client into plaintexts, then flashe_combine_batch_sum_dev with the masks.
    present=[positions] (a round in which clients dropped out: the strictly ascending local positions of the clients that report, one
    Weights each; ValueError for a list that is unsorted, repeats a client, is negative or of another length) keeps every rule above with
    C = the clients present.  Positions in SEVERAL runs ({0,1,3,4}) still take "cohort-chain" at int_bits > 64
    (flashe_quantize_encrypt_cohort_runs_dev / flashe_quantize_batch_encrypt_cohort_runs_dev: present + runs PRF streams, at most 144 of
    them) and "prepared-cohort" with the present clients' masks, and a cohort of more than 144 streams runs "staged-chain".  A gapped
    COMPACT cohort depends on compact_runs, whether the engine has the gapped compact launch
    (flashe_quantize_encrypt_cohort_runs_u32_dev): False (the default) plans it "staged-chain" -- the compact chain then takes one run
    only --, True lets it through to the 144-stream rule like the wide one.  present=None and present=all positions give equal plans,
    whatever compact_runs says.
    cut=True (FlasheCohort(cut=True) on an engine with flashe_quantize_encrypt_cohort_cut_dev) answers
      "cut-chain"     for a shape whose ONLY obstacle above is "the vector does not fill the chip uncut" -- double mask, not batched, one
                      run of consecutive clients, every layer float64 for all clients or for none, at most 128 clients: the summed
                      chain cut into CohortPlan.parts runs of consecutive clients (cohort_cut_parts) and one combine pass, two launches
                      whatever C is (one when parts == 1) and no plaintext in HBM.  A short cohort that is batched, gapped or mixed
                      stays "staged-chain", and so does everything the rules above send there for another reason.
    cut=False: the plans are what they always were.
    cut_any=True beside cut=True (FlasheCohort(cut="any") on an engine with the flashe_*_cohort_cut_runs_* entry points) widens that:
      "cut-chain"     also for a short cohort whose present clients form 2 .. 16 runs, wide and compact -- every gap is a cut the round
                      imposes, the pieces are cohort_cut_pieces' and never fewer than two --, and for a short BATCHED cohort at
                      int_bits > 64 with bs 5, 6 or 7, in one run or several (the rule counts the batched elements).  A cohort of more
                      than 16 runs (one table holds 16 chains) and a mixed-float64 one stay "staged-chain".
    cut_any=False: every plan is what it is without the keyword.
    one_limb=True (FlasheCohort(one_limb=True) on an engine with flashe_quantize_encrypt_cohort_u64_dev) at int_bits 33 .. 64 in the one-limb
    layout replaces the rule "int_bits <= 64" by the compact chain's: "cohort-chain" (uint64 ciphertexts and their sum from the floats, no
    decrypt mask) for a double-mask, un-batched cohort of at most 128 clients in ONE run of consecutive clients whose model has at least
    compact_cohort_admission_length(cu_count, int_bits, n_jobs) values and fewer than 2^32, every layer float64 for all clients or for
    none; a shorter model stays "staged-chain" (the cut launch does not take these widths).  A round in which clients dropped out in
    several runs depends on limb_runs, whether the engine has the gapped one-limb launch (flashe_quantize_encrypt_cohort_runs_u64_dev):
    False (the default) plans it "staged-chain" -- the one-limb chain then takes one run only --, True lets it through to the 144-stream
    rule and the mixed-float64 rule like a compact cohort with compact_runs=True.  Other widths and one_limb=False: every plan is what it
    is without the keywords.
    Touches no device.  The library's own answer stays the last word: a "cohort-chain" or "cut-chain" plan it declines runs
    "staged-chain", a "prepared-cohort" one "prepared-staged"."""
    if len(weights_list) < 1:
        raise ValueError("a cohort needs at least one client's Weights")
    C = len(weights_list)
    present, runs = _present_runs(present, C)
    num_clients = C if num_clients is None else int(num_clients)
    if n_jobs is None:
        from . import cipher as _cipher_mod
        n_jobs = _cipher_mod.N_JOBS

    def dense_clients():
        for c, w in enumerate(weights_list):
            if "zzz" in w._weights or location_masks:
                raise TypeError(f"client {c}: sparse uploads (a 'zzz' layer or location masks) are not supported by FlasheCohort")
            yield list(w.walking_order), w._weights
    names, shapes, _f64, mixed = _one_model(dense_clients())
    sizes = [_size(shp) for shp in shapes]
    starts, n = [], 0
    for s_ in sizes:
        starts.append(n)
        n += s_
    n_elems, bs = n, 1
    if batch:
        bs = int_bits // _field_bits(element_bits, num_clients)
        n_elems = sum((s_ + bs - 1) // bs for s_ in sizes)
    short, parts = False, 1                         # short: the length rule alone keeps the shape from the uncut chain
    limb = bool(one_limb) and not compact and 33 <= int_bits <= 64      # the one-limb chain: the compact chain's rules at these widths
    if cohort_masks and mask == "double":
        if mixed:
            path, reason = PREPARED_STAGED, "a layer is float64 for some clients only: no shared row of one compute class"
        elif batch and compact:
            path, reason = PREPARED_STAGED, "batched job in the compact layout"
        else:
            path, reason = PREPARED_COHORT, "the cohort holds its clients' precomputed masks"
    elif precompute:
        path, reason = PER_CLIENT, "precomputed masks are held per client"
    elif mask not in ("double", "single"):
        path, reason = PER_CLIENT, f"mask {mask!r}"
    elif mask != "double":
        path, reason = STAGED_CHAIN, "single mask: no stream is shared"
    elif compact and int_bits not in _COMPACT_COHORT_WIDTHS:
        path, reason = STAGED_CHAIN, f"int_bits {int_bits} is not a width of the compact chain {_COMPACT_COHORT_WIDTHS}"
    elif not compact and not limb and int_bits <= 64:
        path, reason = STAGED_CHAIN, "int_bits <= 64"
    elif batch and (compact or limb):
        path, reason = STAGED_CHAIN, "batched job"
    elif batch and bs not in _COHORT_BATCH_SIZES:
        path, reason = STAGED_CHAIN, f"batched job with bs {bs}: the chained launch packs {_COHORT_BATCH_SIZES} values per element"
    elif C > _COHORT_MAX_LINKS:
        path, reason = STAGED_CHAIN, f"more than {_COHORT_MAX_LINKS} clients"
    elif not chain:
        path, reason = STAGED_CHAIN, "FLASHE_CHAIN=0"
    elif (compact or limb) and (n >= 2 ** 32 or compact_cohort_blocks(n, int_bits, n_jobs) < 2 * 128 * 16 * int(cu_count)):
        path, reason, short = STAGED_CHAIN, "the vector does not fill the chip uncut", bool(compact) and 1 <= n < 2 ** 32
    elif not compact and not limb and (n_elems < cohort_admission_length(cu_count) or n_elems > 2 ** 32):
        path, reason, short = STAGED_CHAIN, "the vector does not fill the chip uncut", 1 <= n_elems < cohort_admission_length(cu_count)
    elif runs > 1 and limb and not limb_runs:
        path, reason = STAGED_CHAIN, f"clients dropped out ({runs} runs of indices): the one-limb chain takes one run of consecutive clients"
    elif runs > 1 and compact and not compact_runs:
        path, reason = STAGED_CHAIN, f"clients dropped out ({runs} runs of indices): the compact chain takes one run of consecutive clients"
    elif C + runs > _COHORT_MAX_STREAMS:
        path, reason = STAGED_CHAIN, f"clients dropped out: {C} clients in {runs} runs need more than {_COHORT_MAX_STREAMS} PRF streams"
    elif mixed:
        path, reason = STAGED_CHAIN, "a layer is float64 for some clients only"
    else:
        path, reason = COHORT_CHAIN, ""
    if cut and cut_any and short:
        # (batched: only the compiled batch sizes at int_bits > 64 get here -- the rules before the length rule sent the others away)
        if mixed:
            reason = "a layer is float64 for some clients only"
        elif runs > _CUT_MAX_PARTS:
            reason = f"clients dropped out ({runs} runs of indices): the cut chain takes at most {_CUT_MAX_PARTS} runs, one table holds as many chains"
        else:
            begins = cohort_cut_pieces(present, cohort_cut_items(n, int_bits, n_jobs, compact, n_elems if batch else None), cu_count)
            if begins:
                path, reason, parts = CUT_CHAIN, "", len(begins) - 1
    elif cut and short:
        # the rules behind the length rule, in their order, in the cut launch's terms (one run, un-batched)
        if batch:
            reason += "; batched job: the cut chain takes un-batched cohorts"
        elif runs > 1:
            reason = f"clients dropped out ({runs} runs of indices): the cut chain takes one run of consecutive clients"
        elif mixed:
            reason = "a layer is float64 for some clients only"
        else:
            path, reason, parts = CUT_CHAIN, "", cohort_cut_parts(C, cohort_cut_items(n, int_bits, n_jobs, compact), cu_count)
    return CohortPlan(names, shapes, sizes, starts, n, n_elems, [c * n for c in range(C)], path, reason, present, runs, parts)


class _CohortLead(FlasheClient):
    """The cohort's one FlasheClient (its quantiser state is the cohort's): the decrypt of the cohort's own sum adds the mask the chained
    launch wrote -- one memory-bound pass -- instead of computing its two PRF streams again."""
    _cohort_mask = None          # (sum's device pointer, mask DeviceVector, iter, add prefixes, minus prefixes): the lists of the present clients' runs

    def _decrypt_floats(self, dv, sizes, mode, add_idx, minus_idx):
        m, q, c = self._cohort_mask, self.quantizer, self.cipher
        if (m is None or mode is not None or dv.ptr != m[0] or c.iter_index != m[2] or list(add_idx) != m[3]
                or list(minus_idx) != m[4] or len(dv) != len(m[1])):
            return super()._decrypt_floats(dv, sizes, mode, add_idx, minus_idx)
        eng, n = c.engine, len(dv)
        if self.batch:
            # (the batched sum: combine + unbatch + `[:size]` + unquantise in one pass, as the parent's decrypt launch + unbatch launch)
            layers, field_bits = self._batched_back_table(sizes, n)
            dout = eng.alloc(max(8 * sum(sizes), 16))
            eng.combine_unbatch_unquantize_model_dev(layers, q.element_bits, field_bits, q.num_clients, dv.buf, m[1].buf, None, n, dout)
            return dout
        table = self._back_table(sizes, n)
        dout = eng.alloc(max(8 * n, 16))
        eng.combine_unquantize_model_dev(n, dv.buf, m[1].buf, None, table, q.element_bits, q.num_clients, dout)
        return dout


class FlasheCohort(object):
    """`n_local` consecutive clients (ciphers first_idx .. first_idx + n_local - 1 of a federation of num_clients) hosted on ONE GPU --
    a federation simulated on one card, or one card's share of it.  The results are those of n_local FlasheClients run one after the
    other in one process -- every ciphertext, their aggregate, decrypt_unquantize's floats, shape_dict, alpha_list and the mean / std
    history, bit for bit -- but the clients' steps run as ONE chained launch where the chain admits the shape: it quantises every client's
    float model, encrypts with the PRF streams consecutive clients share (n_local + 1 instead of 2 n_local) and writes their sum and the
    decrypt mask, and one memory-bound pass turns the sum into the new float model.  All clients share one quantiser state (every
    client's mean / std / alpha history derives from the same global model).  `path` of the result names the form that ran.
    A batched job at int_bits > 64 whose elements hold 5, 6 or 7 values (element_bits 16 at int_bits 120 / 128) chains too, over its batched
    elements (flashe_quantize_batch_encrypt_cohort_dev), and the decrypt of its own sum is one combine + unbatch + unquantise pass.
    compact=True (int_bits <= 32 on an engine whose compact_supported() is true; ValueError otherwise): every ciphertext and the sum are
    compact DeviceVectors (uint32, elem_bytes 4) whatever path ran, and at int_bits 16 / 20 / 23 / 24 / 32 -- the widths the shipped jobs
    run -- the chained launch goes from the floats to the uint32 ciphertexts and their sum (flashe_quantize_encrypt_cohort_u32_dev: 16
    bytes moved per value and client instead of 36).  No decrypt mask is kept at these widths: decrypt_unquantize() decrypts the
    sum.
    one_limb=True (opt-in, like compact; int_bits 33 .. 64, ValueError otherwise; an engine without the entry point behaves as
    one_limb=False): the widths of a job that quantises finer than the compact chain carries -- element_bits 32 with 2 .. 10 clients,
    int_bits 64 -- chain from the floats too (flashe_quantize_encrypt_cohort_u64_dev: 20 bytes moved per value and client instead of 36).
    The ciphertexts and the sum are the ordinary one-limb DeviceVectors of these widths whatever path ran; no decrypt mask is kept, and
    decrypt_unquantize() decrypts the sum with the telescoped lists.  A model shorter than compact_cohort_admission_length(...), a batched
    job and the single mask stay "staged-chain".
    cut=True (opt-in, like compact): a model too SHORT for the uncut chain -- fewer than cohort_admission_length(cu_count) values, or
    compact_cohort_admission_length(...) in the compact layout: many clients with a small model -- runs "cut-chain" instead of
    "staged-chain": the summed chain cut into runs of consecutive clients and one combine pass (flashe_quantize_encrypt_cohort_cut_dev /
    its _u32 form), two launches whatever n_local is, no plaintext in HBM, the same bytes, and the same decrypt mask kept for
    decrypt_unquantize().  Short cohorts that are batched, gapped (present= in several runs), single-mask, at int_bits 33 - 64 or of more
    than 128 clients stay "staged-chain".
    cut="any" (opt-in; an engine without the entry points behaves as cut=True): "cut-chain" also for a short cohort in which clients
    DROPPED OUT -- present= in 2 .. 16 runs, wide and compact: every gap is a cut, flashe_quantize_encrypt_cohort_cut_runs_dev / its _u32
    form -- and for a short BATCHED cohort at int_bits > 64 with 5, 6 or 7 values per element, in one run or several
    (flashe_quantize_batch_encrypt_cohort_cut_runs_dev).  The wide forms keep the decrypt mask of the telescoped lists, so
    decrypt_unquantize() of such a round stays one combine (+ unbatch) pass; the compact form keeps none.  Any other value of cut:
    ValueError.
    A round in which clients DROPPED OUT is quantize_encrypt(..., present=[positions]): the present clients' steps one after the other, and
    at int_bits > 64 still one chained launch (flashe_quantize_encrypt_cohort_runs_dev / flashe_quantize_batch_encrypt_cohort_runs_dev)
    over present + runs PRF streams that writes the decrypt mask of the telescoped index lists, so decrypt_unquantize() of that round
    stays one pass.  A gapped compact cohort at int_bits 16 / 20 / 23 / 24 / 32 is one chained launch too
    (flashe_quantize_encrypt_cohort_runs_u32_dev, the same streams), on an engine that has it, and so is a gapped one_limb=True cohort
    at int_bits 33 .. 64 (flashe_quantize_encrypt_cohort_runs_u64_dev); no mask is kept there, and decrypt_unquantize() decrypts the sum
    with the telescoped lists.
    A precompute job ("precompute": {"enable": true}) calls prepare_encrypt() in idle time: the next round's masks of all clients as one
    chain of n_local + 1 streams, held by the cohort; the next quantize_encrypt is then ONE online launch with no AES ("prepared-cohort")
    at any int_bits, batched or not, compact or not.  Without that call the clients' own masks run "per-client" as before.  Un-batched and
    with rng= generators over np.random.Philox that launch also generates the stochastic-rounding draws (CohortUpload.draws == "inline":
    no draw buffer in HBM); every other cohort materialises its draws first ("buffer").  inline_draws=True (opt-in, as compact= and cut=
    are) lets a BATCHED precompute job do the same in the shape classes where the measurement says it wins.  inline_draws="any" (as
    cut="any" is to cut=True) does all of that and lets an un-batched "prepared-cohort" round whose generators are all over
    np.random.PCG64 -- np.random.default_rng's -- or all over np.random.PCG64DXSM draw inside its launch too
    (flashe_quantize_combine_cohort_pcg64_dev), under FLASHE_INLINE_DRAWS=1 and in the layouts where _INLINE_PCG64_DEFAULT says so.  Any
    other string: ValueError.
    A DENSE job's arbiter adds the clients' bit-packed models as one integer (jzf_aggregator.py:406-419); CohortUpload.partial_sum is
    the element-wise sum.  aggregate_packed() is that packed reduce of an upload, one pass over the ciphertexts where they lie, and
    decrypt_unquantize(packed=True) decrypts it, so that a cohort which simulates a dense job returns the global model the job produces."""

    def __init__(self, args, first_idx, n_local, num_clients, prp_seed, device=0, stream=None, compact=False, cut=False, inline_draws=False,
                 one_limb=False):
        if isinstance(inline_draws, str) and inline_draws != "any":
            raise ValueError(f"inline_draws: True, False or \"any\", got {inline_draws!r}")
        if n_local < 1 or first_idx < 0 or first_idx + n_local > num_clients:
            raise ValueError(f"clients {first_idx} .. {first_idx + n_local - 1} are not clients of a federation of {num_clients}")
        self.first_idx, self.n_local, self.num_clients = int(first_idx), int(n_local), int(num_clients)
        self.lead = _CohortLead(args, device=device, stream=stream)
        self.lead.create_cipher(self.first_idx, self.num_clients, prp_seed)
        self.compact = bool(compact)
        if isinstance(cut, str) and cut != "any" or not isinstance(cut, str) and cut not in (True, False):
            raise ValueError(f"cut: True, False or \"any\", got {cut!r}")
        self.cut = bool(cut)                           # a short cohort runs "cut-chain" where the engine has the cut launch
        self.inline_draws = bool(inline_draws)         # a BATCHED "prepared-cohort" round may draw inside its online launch (_inline_draws)
        self.inline_any = inline_draws == "any"        # ... and an un-batched one over PCG64 / PCG64DXSM generators (_inline_pcg64_draws)
        self.cut_any = cut == "any"                    # ... gapped or batched too, where the engine has the launches that take indices
        self._cut_scratch = None                       # the cut launch's scratch, kept from round to round
        if self.compact:
            if self.lead.int_bits > 32:
                raise ValueError(f"compact=True needs int_bits <= 32, this job runs int_bits {self.lead.int_bits}")
            ask = getattr(self.lead.cipher.engine, "compact_supported", None)
            if ask is None or not ask():
                raise ValueError("compact=True needs an engine with the uint32 entry points (the table PRF backend, FLASHE_CHAIN not 0)")
        if one_limb and not 33 <= self.lead.int_bits <= 64:
            raise ValueError(f"one_limb=True needs int_bits 33 .. 64, this job runs int_bits {self.lead.int_bits}")
        # the chained launch from the floats at int_bits 33 .. 64, where the engine has it (else the cohort is what it is without the keyword)
        self.one_limb = bool(one_limb) and hasattr(self.lead.cipher.engine, "quantize_encrypt_cohort_u64_dev")
        self._clients = None
        if self.lead.precompute:                       # precomputed masks are per cipher: every client its own, one quantiser state
            self._clients = [self.lead]
            for c in range(1, self.n_local):
                cl = FlasheClient(args, device=device, stream=stream)
                cl.create_cipher(self.first_idx + c, self.num_clients, prp_seed)
                cl.quantizer = self.lead.quantizer
                self._clients.append(cl)
        self._masks = None                             # the cohort's own encrypt-mask cache (prepare_encrypt): one vector per client
        self._last = None                              # the last upload (its sum is what decrypt_unquantize() decrypts)
        self._degrees = None                           # the present clients' degrees of the last quantize_encrypt (None: it took none)
        self.prefer = None                            # "staged-chain" / "per-client": run that fallback form where the chain would be taken (A/B runs)

    quantizer = property(lambda self: self.lead.quantizer)
    cipher = property(lambda self: self.lead.cipher)
    shape_dict = property(lambda self: self.lead.shape_dict)

    def set_iter_index(self, iter_index):
        for cl in (self._clients or [self.lead]):
            cl.cipher.set_iter_index(iter_index)
        self.lead.quantizer.set_iter(iter_index)
        self.lead._cohort_mask = None
        self._last = None

    def plan(self, weights_list, present=None):
        """plan_cohort with this cohort's settings and the engine's CU count (present: quantize_encrypt's)."""
        from . import cipher as _cipher_mod
        ld = self.lead
        if present is not None and _present_runs(present, len(weights_list))[0][-1:] >= [self.n_local]:
            raise ValueError(f"present: the cohort holds positions 0 .. {self.n_local - 1}")
        return plan_cohort(weights_list, ld.int_bits, ld.cipher.engine.cu_count, element_bits=ld.quantizer.element_bits, batch=bool(ld.batch),
                           mask=ld.cipher.masking_scheme, num_clients=self.num_clients, precompute=bool(ld.precompute),
                           chain=os.environ.get("FLASHE_CHAIN", "1") != "0", location_masks=ld.cipher.masks is not None, compact=self.compact,
                           n_jobs=_cipher_mod.N_JOBS, cohort_masks=self._masks is not None, present=present,
                           compact_runs=hasattr(ld.cipher.engine, "quantize_encrypt_cohort_runs_u32_dev"),
                           cut=self.cut and hasattr(ld.cipher.engine, "quantize_encrypt_cohort_cut_u32_dev" if self.compact
                                                    else "quantize_encrypt_cohort_cut_dev"),
                           cut_any=self.cut_any and all(hasattr(ld.cipher.engine, name) for name in self._cut_any_methods()),
                           one_limb=self.one_limb, limb_runs=hasattr(ld.cipher.engine, "quantize_encrypt_cohort_runs_u64_dev"))

    def _cut_any_methods(self):
        """The engine methods cut="any" needs for this cohort's layout."""
        if self.compact:
            return ("cohort_cut_pieces", "quantize_encrypt_cohort_cut_runs_u32_dev")
        return ("cohort_cut_pieces", "quantize_batch_encrypt_cohort_cut_runs_dev" if self.lead.batch else "quantize_encrypt_cohort_cut_runs_dev")

    def prepare_encrypt(self):
        """A precompute job's idle-time step for the whole cohort.  Double mask: the encrypt masks of iteration iter_index + 1 for all
        n_local clients as ONE chain of n_local + 1 PRF streams (consecutive clients share a stream: Engine.cohort_masks_dev) over
        cipher.num_params elements, one vector per client held by the cohort -- compact (uint32) when the cohort is -- in place of the
        clients' own add and minus vectors: masks the clients had prepared themselves are DISCARDED (FlasheCipher.discard_prepared_encrypt),
        as a new prepare_encrypt overwrites them.  The next quantize_encrypt
        consumes them in one online launch ("prepared-cohort").  Single mask (the reference does not read the cache there) or precompute
        off: the clients' own prepare_encrypt."""
        from . import cipher as _cipher_mod
        from .engine import DeviceVector
        ld = self.lead
        c = ld.cipher
        if not ld.precompute or c.masking_scheme != "double":
            for cl in (self._clients or [ld]):
                cl.prepare_encrypt()
            return
        (c.iter_index + 1).to_bytes(4, 'big')                              # same range check as FlasheCipher.prepare_encrypt
        eng, n = c.engine, int(c.num_params)
        masks = [DeviceVector(eng, n, 1, elem_bytes=4) if self.compact else DeviceVector(eng, n) for _ in range(self.n_local)]
        eng.cohort_masks_dev(c.iter_index + 1, self.first_idx, self.n_local, n, _cipher_mod.N_JOBS, [m.buf for m in masks], compact=self.compact)
        eng.sync()
        for m in masks:
            m.mark_ready()
        for cl in self._clients:
            cl.cipher.discard_prepared_encrypt()
        self._masks = masks

    def prepare_decrypt(self):
        """The lead client's prepare_decrypt: the decrypting party's masks do not depend on the cohort."""
        self.lead.prepare_decrypt()

    def quantize_encrypt(self, weights_list, normalize=False, seeds=None, present=None, rng=None, degrees=None):
        """degrees (new): one degree per (present) client, FlasheClient.quantize_encrypt's `degree` of that client (jzf_aggregator.py:676);
        another length or a value that call refuses: ValueError before anything is touched.  Host layers are multiplied on the host; the
        tensors of ALL clients are multiplied and normalised by ONE stage pass (flashe_stage_layers_dev: a row per client and layer) and
        the launches below read its output as plain layers.  A layer that becomes float64 for some clients only (degrees of mixed scalar
        types) takes the staged form, as any layer that computes in float64 for some clients only does.  The cohort remembers them for
        decrypt_unquantize.

        rng (new): the stochastic-rounding draws come from the caller's own np.random.Generator(s) -- ONE Generator: the (present) clients
        draw one after the other from it, as seeds=None does with the global stream; a list of one Generator per (present) client: client c
        draws from rng[c], as seeds=[...] does.  The result is that of the same call with every np.random.random(k) replaced by the
        generator's .random(k), on every path; NumPy's global stream is neither read nor advanced.  Generators over np.random.Philox,
        np.random.PCG64 (np.random.default_rng) or np.random.PCG64DXSM with DEVICE_RNG_MIN draws or more generate on the device, the
        whole cohort in ONE asynchronous launch per kind whatever C is (flashe_philox_random_dev, flashe_pcg64_random_dev), and get their advanced states back; others draw on the host.  rng with seeds, a list of another length:
        ValueError; anything that is not a Generator: TypeError -- before anything is touched.

        One Weights per client (host arrays and / or framework float device tensors, as FlasheClient.quantize_encrypt takes them) ->
        CohortUpload.  present=[positions]: a round in which clients DROPPED OUT -- the strictly ascending local positions (0 .. n_local - 1)
        of the clients that report; weights_list and seeds then hold one entry per present client, the result is that of the present
        clients' FlasheClient steps run one after the other (the p-th present client takes draws [p n, (p + 1) n), absent clients draw
        nothing), CohortUpload.present names their global indices, and where the chain admits the shape the round is still ONE chained
        launch over present + runs PRF streams that writes the decrypt mask of the telescoped index lists.  present=None: everyone, the
        call as it always was.  seeds=None: the stochastic-rounding draws come from NumPy's global stream in client order (client c takes draws
        [c n, (c + 1) n) and the generator is left where n_local sequential steps leave it); seeds=[s_0 ..]: client c draws after
        np.random.seed(s_c), as separate processes would.  The draws of all clients are materialised in HBM (8 bytes each: 2.3 GB for ten
        29.2 M-parameter models), on the device under quantize_encrypt's conditions (MT19937, DEVICE_RNG_MIN) -- except on the path
        "prepared-cohort" of an un-batched job whose rng= generators are all over np.random.Philox: its online launch generates the draws
        itself (flashe_quantize_combine_cohort_philox_dev: a lane's four values are one Philox block of its client's stream), no draw
        buffer is allocated, written or read, whatever the model's length (no DEVICE_RNG_MIN: there is no extra launch to amortise), and
        CohortUpload.draws says "inline" instead of "buffer".  FLASHE_INLINE_DRAWS=0 (read per call) or FLASHE_DEVICE_RNG=0 keeps the
        buffer; so do the staged form and every other generator; the bytes are the same either way.  A BATCHED job keeps the buffer
        unless the cohort was made with inline_draws=True: its online launch then generates the draws too
        (flashe_quantize_batch_combine_cohort_philox_dev: a lane owns four elements and computes each Philox block of their 4 bs values
        once) in the shape classes where that form won its measurement (_INLINE_BATCHED_DEFAULT), and in every class under
        FLASHE_INLINE_DRAWS=1.  A cohort made with inline_draws="any" also draws inside an UN-BATCHED "prepared-cohort" launch when
        every (present) generator is over np.random.PCG64 (np.random.default_rng's) or every one over np.random.PCG64DXSM
        (flashe_quantize_combine_cohort_pcg64_dev: a lane keeps one jump of the LCG for all clients; _inline_pcg64_draws).  Mismatched Weights raise
        ValueError and unusable tensors are refused before anything is launched.  Own-stream engines keep the tensors alive until the
        last kernel that reads them has finished."""
        from .engine import DeviceVector
        ld = self.lead
        q, eng = ld.quantizer, ld.cipher.engine
        plan, layers, pre = self._collect(weights_list, seeds, present, rng, degrees)
        C = len(plan.present)
        rng = _check_rng(rng, C)
        self._refuse_prepared_len(plan, seeds, rng)
        self._last, ld._cohort_mask = None, None
        self._degrees = None if degrees is None else list(degrees)
        ld.degree = None if degrees is None else degrees[0]
        path = self._choose_path(plan, layers)
        if path == PER_CLIENT:
            return self._per_client(weights_list, normalize, seeds, plan.present, rng, degrees)
        if not ld._fusable():
            raise TypeError("FlasheCohort needs the fused client step (fuse=True, a keyed cipher, no location masks)")
        alphas = self._begin_round(plan)
        tables, keep = self._tables(plan, layers, alphas, normalize, degrees if pre is not None else None, pre)
        # (a prepared cohort over Philox generators draws inside its online launch: no draw buffer; a batched one where it asked to)
        inline = path == PREPARED_COHORT and _inline_draws(eng, rng, bool(ld.batch), self.compact, C, plan.n, inline_batched=self.inline_draws,
                                                           bs=ld.int_bits // _field_bits(q.element_bits, q.num_clients) if ld.batch else 0)
        pcg64 = not inline and path == PREPARED_COHORT and self.inline_any and _inline_pcg64_draws(eng, rng, bool(ld.batch), self.compact)
        inline = inline or pcg64
        du = None if inline else _cohort_draws(eng, C, plan.n, seeds, rng)
        if self.compact:
            cts = [DeviceVector(eng, plan.n_elems, 1, elem_bytes=4) for _ in range(C)]
            psum = DeviceVector(eng, plan.n_elems, 1, elem_bytes=4)
        else:
            cts = [DeviceVector(eng, plan.n_elems) for _ in range(C)]
            psum = DeviceVector(eng, plan.n_elems)
        prepared = path in (PREPARED_COHORT, PREPARED_STAGED)       # (the cohort's cache is consumed whatever form runs)
        if path in (COHORT_CHAIN, PREPARED_COHORT, CUT_CHAIN):
            # the shared rows name the compute type; the sources keep their own storage dtypes
            # (with degrees on tensors the tables name the stage pass's output: its code is the compute type)
            rows = [(st, None, al, sh, code if pre is not None else _lib.TENSOR_F64 if layers[0][li][2] == np.float64 else _lib.TENSOR_F32, fl)
                    for li, (st, _p, al, sh, code, fl) in enumerate(tables[0])]
            srcs = [[t[1] for t in table] for table in tables]
            dts = [[t[4] for t in table] for table in tables]
            launch = self._launch_prepared if prepared else self._launch_chain
            if inline and not self._launch_prepared_inline(plan, rows, srcs, dts, rng, cts, psum, pcg64):
                # the library declined the inline form: today's form, from the same generators (nothing has been advanced)
                inline, du = False, _cohort_draws(eng, C, plan.n, seeds, rng)
            if not inline and not launch(plan, rows, srcs, dts, du, cts, psum, present is not None, **({"cut": True} if path == CUT_CHAIN else {})):
                # the library declined: the planner's guess was wrong, the result is not -- the same bytes from the fallback form
                path = PREPARED_STAGED if prepared else STAGED_CHAIN
        if path in (STAGED_CHAIN, PREPARED_STAGED) and plan.n_elems:
            cts, psum, held = self._launch_staged(plan, tables, du, cts, psum, prepared)
            keep += held
        if prepared:
            keep += list(self._masks)
            self._masks = None                         # consumed by this call, whatever the iteration (the reference does not check it either)
        eng.hold(keep + ([] if du is None else [du]))
        if ld.batch:
            bs = ld.int_bits // _field_bits(q.element_bits, q.num_clients)
            q.shape_list = list(plan.shapes)
            ld.shape_dict = {k: ((s_ + bs - 1) // bs,) for k, s_ in zip(plan.names, plan.sizes)}
        else:
            ld.shape_dict = dict(zip(plan.names, plan.shapes))
        for v in cts:
            v.mark_ready()
        psum.mark_ready()
        self._last = CohortUpload(cts, psum, path, [self.first_idx + p for p in plan.present], draws="inline" if inline else "buffer")
        return self._last

    def _collect(self, weights_list, seeds, present=None, rng=None, degrees=None):
        """(plan, every layer of every present client as _layer_source gives it, pre): the refusals, before anything of the cohort's state
        is touched.  With degrees a host layer is `layer * degree` already and a tensor's NumPy dtype is the one that product has;
        pre[c][l] = the tensor's dtype before it (None for a host layer: nothing left to multiply), pre = None without degrees or
        without a tensor."""
        C = self.n_local if present is None else len(weights_list)
        if len(weights_list) != C:
            raise ValueError(f"the cohort holds {C} clients, got {len(weights_list)} Weights")
        if seeds is not None and len(seeds) != C:
            raise ValueError(f"seeds: one per client ({C}), got {len(seeds)}")
        if rng is not None and seeds is not None:
            raise ValueError("rng and seeds: one source of draws at a time")
        _check_rng(rng, C)
        if degrees is not None:
            if len(degrees) != C:
                raise ValueError(f"degrees: one per client ({C}), got {len(degrees)}")
            for ci, d in enumerate(degrees):
                if _check_degree(d, f"degrees[{ci}]") is None:
                    raise ValueError(f"degrees[{ci}] is None: every present client has a degree, or degrees=None")
        plan = self.plan(weights_list, present)
        eng = self.lead.cipher.engine
        if degrees is None:
            return plan, [[_layer_source(eng, w._weights[k], f"client {ci} layer {k!r}") for k in plan.names] for ci, w in enumerate(weights_list)], None
        if not hasattr(eng, "stage_layers_dev") and any(interop.is_foreign(w._weights[k]) for w in weights_list for k in plan.names):
            raise TypeError("degrees with framework tensors need an engine with flashe_stage_layers_dev")
        layers, pre = [], []
        for ci, w in enumerate(weights_list):
            row, before = [], []
            for k in plan.names:
                v = w._weights[k]
                if interop.is_foreign(v):
                    x, code, hdt, size, shape = _layer_source(eng, v, f"client {ci} layer {k!r}")
                    row.append((x, code, _loop_dtype(hdt, degrees[ci]), size, shape))
                    before.append(hdt)
                else:
                    row.append(_layer_source(eng, np.asarray(v) * degrees[ci], f"client {ci} layer {k!r}"))
                    before.append(None)
            layers.append(row)
            pre.append(before)
        # (host layers only: they are multiplied already, nothing of the step changes)
        return plan, layers, pre if any(b is not None for before in pre for b in before) else None

    def _refuse_prepared_len(self, plan, seeds, rng=None):
        """A cache of another length: the call-by-call step's ValueError, where the first sequential client raises it (after its quantiser
        has drawn one value per model value, FlasheClient._refuse_prepared_len); the cache stays, and nothing of the cohort's state has
        been touched or uploaded yet."""
        if self._masks is None or plan.path not in (PREPARED_COHORT, PREPARED_STAGED) or len(self._masks[0]) == plan.n_elems:
            return
        if seeds is not None:
            np.random.seed(seeds[0])
        _skip_draws(plan.n, _client_rng(rng, 0))
        self.lead.cipher._check_prepared_len(self._masks[0], plan.n_elems)

    def _choose_path(self, plan, layers):
        """The plan's path after what only the layers themselves and `prefer` tell."""
        path = plan.path
        if any(layer[2] != first[2] for row in layers for layer, first in zip(row, layers[0])) and path in (COHORT_CHAIN, PREPARED_COHORT, CUT_CHAIN):
            # (a layer that computes in float64 for some clients only: no shared row)
            path = PREPARED_STAGED if path == PREPARED_COHORT else STAGED_CHAIN
        prepared = path in (PREPARED_COHORT, PREPARED_STAGED)       # (the cohort's cache is consumed whatever `prefer` says)
        if prepared and self.prefer == STAGED_CHAIN:
            return PREPARED_STAGED
        if not prepared and (self.prefer == PER_CLIENT or (self.prefer == STAGED_CHAIN and path in (COHORT_CHAIN, CUT_CHAIN))):
            return self.prefer
        return path

    def _begin_round(self, plan):
        """The one quantiser state -- set_layer_size_list and r_max_list / alpha_list of this round, as FlasheClient's tensor step leaves
        them -- and the cipher's encrypt prefixes.  Returns the alphas."""
        q = self.lead.quantizer
        alphas = _round_alphas(q, plan.sizes)
        q.r_max_list = [alphas[li] * q.num_clients for li in range(len(plan.names))]
        q.alpha_list = [alphas[li] for li in range(len(plan.names))]
        self.lead.cipher.set_idx_list(mode="encrypt")
        return alphas

    def _tables(self, plan, layers, alphas, normalize, degrees=None, pre=None):
        """(every client's tensor-layer table, keep): host layers go up once, client by client.  With degrees: ONE stage pass for all
        clients (_stage_scaled), and the tables name its output as plain layers."""
        eng, means = self.lead.cipher.engine, self.lead.quantizer.past_layer_mean_list
        tables, keep = [], []
        if degrees is not None:
            items = []
            for ci, row in enumerate(layers):
                ptrs, held = _stage_host_layers(eng, [layer[0] for layer in row])
                keep += held
                for li, (_x, code, hdt, size, _shape) in enumerate(row):
                    tensor = pre[ci][li] is not None
                    items.append((ptrs[li], code, pre[ci][li] if tensor else hdt, size, degrees[ci] if tensor else None, alphas[li],
                                  means[li] if normalize else None))
            staged, scratch = _stage_scaled(eng, items)
            keep.append(scratch)
            L = len(plan.names)
            for ci in range(len(layers)):
                tables.append([(plan.starts[li], staged[ci * L + li][0], alphas[li], 0.0, staged[ci * L + li][1], 0) for li in range(L)])
            return tables, keep
        for row in layers:
            ptrs, held = _stage_host_layers(eng, [layer[0] for layer in row])
            keep += held
            table = []
            for li, (_x, code, hdt, _size, _shape) in enumerate(row):
                shift, flags = _tensor_flags(hdt, alphas[li], normalize, means[li])
                table.append((plan.starts[li], ptrs[li], alphas[li], shift, code, flags))
            tables.append(table)
        return tables, keep

    def _launch_chain(self, plan, rows, srcs, dts, du, cts, psum, by_idx=False, cut=False):
        """"cohort-chain": ONE chained launch from the floats to the ciphertexts, their sum and -- when the cohort is the whole federation --
        the decrypt mask, which the lead keeps with the add / minus lists it stands for, for the decrypt of that sum.  by_idx (a call with
        `present`): the launch is given the present clients' cipher indices, any number of runs.  cut ("cut-chain", one run of clients):
        the chain cut into the library's cohort_cut_parts pieces plus the combine pass, with the scratch the pieces' sums and masks go
        through; the outputs and the mask kept are those of the uncut launch.  A gapped or batched "cut-chain" (cut="any") goes through
        the launches that take the cipher indices, with the library's cohort_cut_pieces count; the mask kept is that of the telescoped
        lists.  False: the library declined, nothing was launched."""
        from . import cipher as _cipher_mod
        from .engine import DeviceVector
        ld = self.lead
        q, c, eng = ld.quantizer, ld.cipher, ld.cipher.engine
        n, n_elems = plan.n, plan.n_elems
        # (no decrypt mask at the compact widths or in the one-limb layout: the decrypt of the sum is 2 / m AES blocks per element)
        narrow = self.compact or self.one_limb
        dmask = DeviceVector(eng, n_elems) if self.n_local == self.num_clients and not narrow else None
        outs, mask_buf = [v.buf for v in cts], dmask.buf if dmask is not None else None
        idxs = [self.first_idx + p for p in plan.present]
        jobs, batch = _cipher_mod.N_JOBS, bool(ld.batch) and not narrow
        # the form: the cipher indices as a list for a gapped or batched cut and for a call with `present` (one run of a compact cohort
        # or one-limb cohort without its gapped launch: plan_cohort sends a gapped one to the staged form), else the first index.  One
        # limb (int_bits 33 .. 64): never cut
        if self.one_limb:
            cut = False
        layout = "_u32" if self.compact else "_u64" if self.one_limb else ""
        by_list = (plan.runs > 1 or bool(ld.batch)) if cut else (by_idx and (not narrow or hasattr(eng, f"quantize_encrypt_cohort_runs{layout}_dev")))
        name = f"quantize_{'batch_' if batch else ''}encrypt_cohort{'_cut' if cut else ''}{'_runs' if by_list else ''}{layout}_dev"
        scratch = ()
        if cut:
            # the library's piece count sizes the scratch: the pieces' sums (compact: uint32) and, behind them, their decrypt masks
            elems = n_elems if by_list else n
            parts = eng.cohort_cut_pieces(idxs, elems, jobs, compact=self.compact)[0] if by_list else eng.cohort_cut_parts(len(idxs), elems, jobs, compact=self.compact)
            if not parts:
                return False
            need = 0 if parts == 1 else parts * elems * (4 if self.compact else 16 * (2 if dmask is not None else 1))
            if need and (self._cut_scratch is None or self._cut_scratch.nbytes < need):
                self._cut_scratch = eng.alloc(max(need, 16))
            scratch = (self._cut_scratch if need else None,)
        took = getattr(eng, name)(c.iter_index, idxs if by_list else idxs[0] if idxs else self.first_idx, *((n, n_elems) if batch else (n,)), jobs, rows,
                                  srcs, dts, q.element_bits, *((_field_bits(q.element_bits, q.num_clients),) if batch else ()), du, outs, psum.buf,
                                  *(() if narrow else (mask_buf,)), *scratch)
        if took and dmask is not None:
            ld._cohort_mask = (psum.ptr, dmask, c.iter_index) + _telescoped(idxs)
        return took

    def _launch_prepared(self, plan, rows, srcs, dts, du, cts, psum, by_idx=False):
        """"prepared-cohort": ONE online launch, every client's floats and its precomputed mask -> its ciphertext, and their sum; no AES.
        False: the library declined, nothing was launched."""
        ld = self.lead
        masks, outs, batch = self._prepared_vectors(plan, cts)
        return ld.cipher.engine.quantize_combine_cohort_dev(plan.n, rows, srcs, dts, ld.quantizer.element_bits, du, masks, outs, psum.buf, compact=self.compact, batch=batch)

    def _prepared_vectors(self, plan, cts):
        """What either "prepared-cohort" launch is given: the present clients' masks, the ciphertexts, and batch= (None: not a batched job)."""
        q, masks = self.lead.quantizer, [self._masks[p].buf for p in plan.present]
        return masks, [v.buf for v in cts], (plan.n_elems, _field_bits(q.element_bits, q.num_clients)) if self.lead.batch else None

    def _launch_prepared_inline(self, plan, rows, srcs, dts, rng, cts, psum, pcg64=False):
        """"prepared-cohort" with the draws generated inside the online launch (_inline_draws; pcg64: _inline_pcg64_draws, the PCG64
        family's call): one Generator gives ONE stretch of C n draws, the p-th present client taking [p n, (p + 1) n); a list client
        p's stretch from rng[p].  The generators get their advanced states back.  False: the library declined or refused the table,
        nothing was launched and nothing advanced."""
        ld = self.lead
        C, n = len(plan.present), plan.n
        gens, counts, offsets = (rng, [n] * C, [p * n for p in range(C)]) if isinstance(rng, list) else ([rng], [C * n], [0])
        masks, outs, batch = self._prepared_vectors(plan, cts)
        eng, bits = ld.cipher.engine, ld.quantizer.element_bits
        if pcg64:
            return eng.quantize_combine_cohort_pcg64_dev(n, rows, srcs, dts, bits, gens, counts, offsets, masks, outs, psum.buf, compact=self.compact)
        return eng.quantize_combine_cohort_philox_dev(n, rows, srcs, dts, bits, gens, counts, offsets, masks, outs, psum.buf, compact=self.compact,
                                                      **({"batch": batch} if batch else {}))

    def _launch_staged(self, plan, tables, du, cts, psum, prepared):
        """A quantise (+ batch) pass per client into plaintexts -- un-batched: one value per element, field_bits = int_bits -- then
        "staged-chain": the summed batch encrypt, which chains where it can; "prepared-staged": the combines with the masks and their sum
        in one pass (one-limb vectors: a compact cohort widens its masks before and narrows the results after).
        Returns (ciphertexts, sum, what the launches read)."""
        from . import cipher as _cipher_mod
        from .engine import DeviceVector
        ld = self.lead
        q, c, eng = ld.quantizer, ld.cipher, ld.cipher.engine
        C, n_elems = len(plan.present), plan.n_elems
        field_bits = _field_bits(q.element_bits, q.num_clients) if ld.batch else ld.int_bits
        pts = [eng.alloc_vec(n_elems) for _ in range(C)]
        for ci in range(C):
            eng.quantize_batch_tensors_dev(tables[ci], plan.n, q.element_bits, field_bits, du.ptr + 8 * plan.draw_offsets[ci], n_elems, pts[ci])
        if prepared:
            adds = [self._masks[p].widened(eng) for p in plan.present]
            wide = [DeviceVector(eng, n_elems) for _ in range(C)] if self.compact else cts
            wsum = DeviceVector(eng, n_elems) if self.compact else psum
            eng.combine_batch_sum_dev(n_elems, pts, eng.limbs, [a.buf for a in adds], None, [v.buf for v in wide], wsum.buf)
            if self.compact:
                cts, psum = [v.mark_ready().narrowed(eng) for v in wide], wsum.mark_ready().narrowed(eng)
            return cts, psum, pts + adds
        idxs = [self.first_idx + p for p in plan.present]
        scheme = 1 if c.masking_scheme == "double" else 0
        if self.compact:
            pts = [DeviceVector(eng, n_elems, 1, buf=pt).narrowed().buf for pt in pts]
            eng.encrypt_batch_sum_u32_dev(c.iter_index, idxs, scheme, n_elems, _cipher_mod.N_JOBS, pts, [v.buf for v in cts], psum.buf)
        else:
            eng.encrypt_batch_sum_dev(c.iter_index, idxs, scheme, n_elems, _cipher_mod.N_JOBS, pts, eng.limbs, [v.buf for v in cts], psum.buf)
        return cts, psum, pts

    def _per_client(self, weights_list, normalize, seeds, present=None, rng=None, degrees=None):
        """The present clients' own steps one after the other (one cipher re-indexed per client; with precompute: every client's own cipher
        and masks), then the aggregate of what they wrote."""
        ld = self.lead
        cts = []
        present = list(range(len(weights_list))) if present is None else present
        try:
            for ci, w in enumerate(weights_list):
                cl = self._clients[present[ci]] if self._clients else ld
                cl.cipher.idx = self.first_idx + present[ci]
                if seeds is not None:
                    np.random.seed(seeds[ci])
                lw = _Layers({k: w._weights[k] for k in w.walking_order})
                lw.walking_order = list(w.walking_order)
                up = cl.quantize_encrypt(lw, device=True, normalize=normalize, **_rng_kw(_client_rng(rng, ci)),
                                         **({} if degrees is None else {"degree": degrees[ci]}))
                ct = up._weights[up.walking_order[0]]
                cts.append(cl.cipher._as_compact(ct) if self.compact else ct)
                ld.shape_dict = cl.shape_dict
        finally:
            ld.cipher.idx = self.first_idx
            ld.degree = None if degrees is None else degrees[0]
        psum = ld.cipher.aggregate(cts, device=True)
        self._last = CohortUpload(cts, psum, PER_CLIENT, [self.first_idx + p for p in present])
        return self._last

    def aggregate_packed(self, upload=None):
        """The arbiter's PACKED reduce (jzf_aggregator.py:406-419: the clients' compressed models added as one integer, carries crossing
        from element j + 1 into element j) of an upload's ciphertexts -- default: the last upload -- as a DeviceVector in the upload's
        layout: what FlasheCipher.aggregate(ciphertexts, packed=True) returns for the clients' own FlasheClient ciphertexts, one pass
        over the unpacked vectors where the engine has it (flashe_aggregate_packed_elems_dev / its _u32 form).  A dense job's arbiter
        reduces this way; CohortUpload.partial_sum is the element-wise sum.  The whole federation's sum is the packed reduce of the
        cohorts' results, so a partial cohort's result is something an arbiter can add on."""
        up = self._last if upload is None else upload
        if up is None:
            raise ValueError("aggregate_packed() needs the upload of this iteration (quantize_encrypt first)")
        from . import cipher as _cipher_mod
        eng = self.lead.cipher.engine
        res = _cipher_mod.aggregate(list(up.ciphertexts), self.lead.int_bits, packed=True, _engine=eng, keep_on_device=True, _compact_result=self.compact)
        return res.narrowed(eng) if self.compact and not res.compact else res

    def decrypt_unquantize(self, aggregate=None, uploaded=None, out=None, unnormalize=False, degree=None, total_degree=None, last_round=None,
                           packed=False):
        """packed=True (new; only without `aggregate`, ValueError otherwise): the cohort's own upload is reduced as a dense job's arbiter
        reduces it -- aggregate_packed() -- and THAT sum is decrypted instead of partial_sum: after a "cohort-chain" / "cut-chain" upload
        still by adding the mask the launch wrote, in one pass (the mask does not depend on which sum it is added to), otherwise with
        the telescoped lists; present= rounds included.

        degree, total_degree, last_round (new): FlasheClient.decrypt_unquantize's, handed to the lead.  When the cohort decrypts its own
        sum and both degrees are omitted after a quantize_encrypt(degrees=...), degree is the first present client's and total_degree the
        left-to-right sum of the present clients' degrees (what the arbiter reduces, jzf_aggregator.py:380).

        The new global model as FlasheClient.decrypt_unquantize returns it (out=: written into the caller's tensors, in place).  Without
        an aggregate: the cohort is the whole federation and its own last partial_sum is decrypted, `uploaded` defaulting to the clients
        that upload held (CohortUpload.present) -- after a "cohort-chain" upload by adding the mask that launch wrote (one memory-bound
        pass) whenever set_idx_list yields exactly the add / minus lists the mask stands for; ValueError when clients outside the cohort
        exist.  With an aggregate (a DeviceVector, limbs, a framework tensor, or Weights holding one): `uploaded` lists the clients it sums
        (default: all num_clients)."""
        ld = self.lead
        own = aggregate is None
        if packed and not own:
            raise ValueError("packed=True decrypts the cohort's own upload: it cannot be combined with aggregate=")
        if aggregate is None:
            if self.n_local != self.num_clients:
                raise ValueError(f"the cohort holds {self.n_local} of {self.num_clients} clients: decrypt_unquantize needs the federation's aggregate")
            if self._last is None:
                raise ValueError("decrypt_unquantize() without an aggregate needs the upload of this iteration (quantize_encrypt first)")
            aggregate = self._last.partial_sum
            if packed:
                aggregate = packed_sum = self.aggregate_packed(self._last)
        if uploaded is None:
            uploaded = list(self._last.present) if own and self._last.present is not None else list(range(self.num_clients))
        if ld.shape_dict is None:
            raise ValueError("decrypt_unquantize needs the layer shapes a quantize_encrypt left behind (shape_dict)")
        if not hasattr(aggregate, "walking_order"):
            aggregate = _Layers({next(iter(ld.shape_dict), "w"): aggregate})
        if own and degree is None and total_degree is None and self._degrees:
            degree, total_degree = self._degrees[0], functools.reduce(operator.add, self._degrees)
        degree, total_degree = ld._back_degrees(degree, total_degree)      # (refused before set_idx_list touches the cipher)
        ld.set_idx_list(list(uploaded))
        kept = ld._cohort_mask
        if packed and kept is not None and kept[0] == self._last.partial_sum.ptr:
            ld._cohort_mask = (packed_sum.ptr,) + kept[1:]      # the mask the launch wrote decrypts the packed sum of the same upload too
        try:
            return ld.decrypt_unquantize(aggregate, out=out, unnormalize=unnormalize, degree=degree, total_degree=total_degree,
                                         last_round=last_round)
        finally:
            ld._cohort_mask = kept


# ---- a cohort of sparse-job clients hosted on one GPU (new) ----------------------------------------------------------------------
SPARSE_COHORT = "sparse-cohort"
FRONT_FUSED, FRONT_STAGED = "fused", "staged"


class SparseCohortPlan(object):
    """What plan_sparse_cohort returns: names / shapes / sizes / starts of the shared DENSE layer table, total (values of one model) and
    bits = total.bit_length(); ks (entries Client.sparsify keeps of every layer: max(1, floor(sparsity * size)), a function of the shape
    only), K = sum(ks), compact_starts (layer l's first compact value), n_elems = K + 1 (elements of one upload), draw_offsets (client
    c's first draw in the client-major draws: c (K + 1), the last of its K + 1 draws is its 'zzz' draw), f64 (does layer l compute in
    float64?), path and the reason for it; front_end ("fused": the uploads come out of ONE chained launch from the floats, "staged": one
    quantise launch into plaintexts, then the encrypts) and front_end_reason, why it is "staged"."""

    def __init__(self, names, shapes, sizes, starts, total, ks, compact_starts, draw_offsets, f64, path, reason, front_end=None, front_end_reason=""):
        self.names, self.shapes, self.sizes, self.starts, self.total, self.bits = names, shapes, sizes, starts, total, int(total).bit_length()
        self.ks, self.K, self.compact_starts, self.n_elems = ks, sum(ks), compact_starts, sum(ks) + 1
        self.draw_offsets, self.f64, self.path, self.reason = draw_offsets, f64, path, reason
        self.front_end, self.front_end_reason = front_end or FRONT_STAGED, front_end_reason


class SparseCohortEncoding(object):
    """FlasheSparseCohort.sparsify's result: encoded (per client what Sparsifier.sparsify returns: (packed locations, K, bits, total)),
    locations (per client (DeviceBuffer of K uint32 model-wide locations, K): what dynamic_masking_choice takes) and compact (per client
    {layer name: CompactLayer}: the kept values where they lie in HBM)."""

    def __init__(self, encoded, locations, compact):
        self.encoded, self.locations, self.compact = encoded, locations, compact


class SparseCohortUpload(object):
    """FlasheSparseCohort.quantize_encrypt's result: uploads (one DeviceVector of K + 1 elements per client: the K ciphertexts and the
    un-encrypted quantised zero), aggregate (aggregate_sparse_uploads of them: `total` elements), path and front_end ("fused" / "staged":
    the form that made the uploads)."""

    def __init__(self, uploads, aggregate, path, front_end=FRONT_STAGED):
        self.uploads, self.aggregate, self.path, self.front_end = uploads, aggregate, path, front_end


def _client_layers(w, walking_order=None):
    """(names in walking order, {name: layer}) of a Weights-like object or a plain dict."""
    if hasattr(w, "_weights"):
        return list(walking_order if walking_order is not None else w.walking_order), w._weights
    return list(walking_order) if walking_order is not None else sorted(w.keys(), key=str), w


def plan_sparse_cohort(weights_list, sparsity, int_bits, element_bits=16, batch=False, choice="single", precompute=False, fuse=True,
                       walking_order=None):
    """The engine-free part of FlasheSparseCohort: checks that the clients' dense models describe ONE model (the same layer names in the
    same walking order with the same shapes: ValueError naming the client and the layer, as plan_cohort; an empty layer: Sparsifier's
    ValueError), lays out the shared layer table, the compact layers and the client-major draws, and picks the path:
      "sparse-cohort"  one set of sparsifier launches, one quantise launch, the fused encrypt + aggregate: choice "single" (what the
                       arbiter's cost rule answers for every sparsifier-fed round), not batched, no precompute cache, fuse, every layer in
                       the same compute class (float64, or float32 / float16 / bfloat16) for all clients.  There is NO minimum size;
      "per-client"     everything else (choice "double" set by hand, batched jobs, precompute, fuse off, a layer that is float64 for some
                       clients only): the clients' own FlasheClient steps on the shared quantiser state, then aggregate_sparse_uploads.
    Touches no device."""
    if len(weights_list) < 1:
        raise ValueError("a cohort needs at least one client's model")
    C = len(weights_list)
    names, shapes, f64, mixed = _one_model(_client_layers(w, walking_order) for w in weights_list)
    sizes = [_size(shp) for shp in shapes]
    for k, size in zip(names, sizes):
        if size == 0:
            raise ValueError(f"layer {k!r} is empty: the sparsifier keeps max(1, floor(sparsity * size)) values of every layer")
    ks = [max(1, int(np.floor(sparsity * size))) for size in sizes]
    starts, total = [], 0
    for s_ in sizes:
        starts.append(total)
        total += s_
    cstarts, K = [], 0
    for k_l in ks:
        cstarts.append(K)
        K += k_l
    path, reason = _sparse_path(choice, batch, precompute, fuse, mixed)
    front, front_reason = _sparse_front_end(path, reason, int_bits, C, K)
    return SparseCohortPlan(names, shapes, sizes, starts, total, ks, cstarts, [c * (K + 1) for c in range(C)], f64, path, reason, front, front_reason)


def _sparse_front_end(path, reason, int_bits, n_clients, K):
    """("fused" | "staged", reason): does flashe_quantize_encrypt_sparse_cohort_dev take the cohort's uploads?  The library's own admission
    rule, without a device (another PRF backend than the table one is the library's to refuse)."""
    if path != SPARSE_COHORT:
        return FRONT_STAGED, reason
    if int_bits not in _COMPACT_COHORT_WIDTHS:
        return FRONT_STAGED, f"int_bits {int_bits} is not one of the chained widths {_COMPACT_COHORT_WIDTHS}"
    if n_clients > _COHORT_MAX_LINKS:
        return FRONT_STAGED, f"{n_clients} clients (the chained launch takes {_COHORT_MAX_LINKS})"
    if K >= 1 << 32:
        return FRONT_STAGED, "2^32 compact values or more"
    if os.environ.get("FLASHE_CHAIN", "1") == "0":
        return FRONT_STAGED, "FLASHE_CHAIN=0"
    return FRONT_FUSED, ""


def _sparse_path(choice, batch, precompute, fuse, mixed):
    if choice != "single":
        return PER_CLIENT, f"masking choice {choice!r} (set by hand: strictly increasing lists always cost 'single')"
    if batch:
        return PER_CLIENT, "batched job"
    if precompute:
        return PER_CLIENT, "precomputed masks are held per client"
    if not fuse:
        return PER_CLIENT, "fuse is off"
    if mixed:
        return PER_CLIENT, "a layer is float64 for some clients only"
    return SPARSE_COHORT, ""


class FlasheSparseCohort(object):
    """`n_local` consecutive clients of the SPARSE job (ciphers first_idx .. first_idx + n_local - 1 of a federation of num_clients)
    hosted on ONE GPU: Client.sparsify -> locations to the arbiter -> dynamic_masking -> Client.secure_aggregate's quantise + encrypt ->
    Arbiter.expand_to_dense + reduce -> Client.aggregate's decrypt + unquantise (jzf_aggregator.py:578-623, 717-743, 881-899;
    jzf_flashe_block.py:92-117; jzf_quantize.py:433-465), one method per step.  Every result is that of n_local Sparsifiers +
    FlasheClients run one after the other in one process on ONE shared quantiser state (FlasheCohort's rule), followed by
    aggregate_sparse_uploads and client first_idx's decrypt_unquantize -- bit for bit -- but the device work of the whole cohort is a
    number of launches that does not grow with n_local: one set of sparsifier launches over a C x L row table
    (flashe_sparsify_cohort_tensors_dev), the uploads in ONE chained launch from the floats at int_bits 16 / 20 / 23 / 24 / 32
    (flashe_quantize_encrypt_sparse_cohort_dev, front_end "fused": no plaintext vector in HBM) followed by the sparse aggregate -- at
    the other widths one quantise launch (flashe_quantize_cohort_dev) and the fused encrypt + aggregate
    (flashe_sparse_encrypt_aggregate_dev; at int_bits <= 64 one batched encrypt launch and the aggregate) -- with the span bounds of
    the round's lists computed once, and the sparse decrypt + unquantise + store.  One engine and one stream carry everything, the sparsifier passes included.  `path` of an upload names the form that ran."""

    def __init__(self, args, first_idx, n_local, num_clients, prp_seed, sparsity, device=0, stream=None):
        if n_local < 1 or first_idx < 0 or first_idx + n_local > num_clients:
            raise ValueError(f"clients {first_idx} .. {first_idx + n_local - 1} are not clients of a federation of {num_clients}")
        if args.get("mask", "double") != "dynamic":
            raise ValueError("FlasheSparseCohort runs the sparse job: args['mask'] must be 'dynamic' (the arbiter's choice reaches the clients)")
        self.first_idx, self.n_local, self.num_clients, self.sparsity = int(first_idx), int(n_local), int(num_clients), sparsity
        self.lead = FlasheClient(args, device=device, stream=stream)
        self.lead.create_cipher(self.first_idx, self.num_clients, prp_seed)
        self._clients = None
        if self.lead.precompute:                       # precomputed masks are per cipher: every client its own, one quantiser state
            self._clients = [self.lead]
            for c in range(1, self.n_local):
                cl = FlasheClient(args, device=device, stream=stream)
                cl.create_cipher(self.first_idx + c, self.num_clients, prp_seed)
                cl.quantizer = self.lead.quantizer
                self._clients.append(cl)
        self.shape_dict_used_for_sparsification = None
        self.plan = None                # of the last sparsify
        self._remain = None             # (DeviceBuffer, names, sizes, per-layer compute dtypes, stride in bytes): C residual blocks in HBM
        self._fallback = None           # per-client Sparsifiers (a layer that is float64 for some clients only)
        self._compact = None            # per client [(ptr, dtype code, NumPy dtype)] of the compact layers + what keeps them alive
        self._own_lists = None          # per client (DeviceBuffer of uint32 locations, K) from the last sparsify
        self._lists = None              # the round's lists of ALL num_clients clients: (DeviceBuffer, k), + are they strictly increasing
        self._sorted = True
        self._host_masks = None
        self._bounds = None             # (SpanBounds of the cohort's own lists, (total, C)): reused over rounds of the same shape
        self._last = None
        self._last_bounds = None        # the handle the decrypt of the cohort's own aggregate may take
        self.prefer_front_end = None    # "staged": quantise into plaintexts, then encrypt, where the chained launch would be taken (A/B runs)

    quantizer = property(lambda self: self.lead.quantizer)
    cipher = property(lambda self: self.lead.cipher)
    shape_dict = property(lambda self: self.lead.shape_dict)
    alpha_list = property(lambda self: self.lead.quantizer.alpha_list)
    engine = property(lambda self: self.lead.cipher.engine)

    def set_iter_index(self, iter_index):
        for cl in (self._clients or [self.lead]):
            cl.cipher.set_iter_index(iter_index)
        self.lead.quantizer.set_iter(iter_index)
        self._last = None

    # ---- Client.sparsify for all clients ---------------------------------------------------------------------------------------
    def sparsify(self, weights_list, walking_order=None):
        """One dense model per client (Weights or dict; host arrays and / or framework float device tensors) -> SparseCohortEncoding.
        Client c's result is its own Sparsifier(sparsity).sparsify(W_c, order): the same (encoded, le, bits, total), compact values and
        residuals as bytes.  The residuals stay in HBM per client between rounds (remain_weights(c) downloads them) and continue a
        previous round; the caller's models are neither written nor replaced.  Everything is checked before a residual is touched."""
        from ._lib import TENSOR_F32, TENSOR_F64
        from .engine import DeviceBufferView
        from .weights import CompactLayer, _compact_layout
        C = self.n_local
        if len(weights_list) != C:
            raise ValueError(f"the cohort holds {C} clients, got {len(weights_list)} models")
        ld = self.lead
        plan = plan_sparse_cohort(weights_list, self.sparsity, ld.int_bits, element_bits=ld.quantizer.element_bits, walking_order=walking_order)
        eng = self.engine
        names, L = plan.names, len(plan.names)
        rows = []                                     # per client [(ForeignArray or flat host array, dtype code)]
        for ci, w in enumerate(weights_list):
            _o, layers = _client_layers(w, walking_order)
            rows.append([_layer_source(eng, layers[k], f"client {ci} layer {k!r}")[:2] for k in names])
        if self.shape_dict_used_for_sparsification is None:
            self.shape_dict_used_for_sparsification = dict(zip(names, plan.shapes))
        self.plan, self._last = plan, None
        if plan.path == PER_CLIENT:                   # (here: a layer that is float64 for some clients only -- no shared row)
            return self._sparsify_per_client(weights_list, walking_order, plan)
        cts = tuple(np.dtype(np.float64 if f else np.float32) for f in plan.f64)
        roffs, rbytes = _compact_layout(plan.sizes, cts)
        voffs, vbytes = _compact_layout(plan.ks, cts)
        rstride, vstride = (rbytes + 15) & ~15, (vbytes + 15) & ~15
        K, bits = plan.K, plan.bits
        lstride = (K + 3) & ~3
        n_limbs = (K * bits + 63) // 64
        # the residuals: C blocks in the layout of the call; another layout (or the per-client form) continues from the host copies
        rem = self._remain
        if rem is None or rem[1] != names or rem[2] != plan.sizes or rem[3] != cts:
            host = [self.remain_weights(ci) for ci in range(C)] if (rem is not None or self._fallback is not None) else None
            buf = eng.alloc(max(C * rstride, 16))
            if host is None or not any(h for h in host):
                eng.memset_dev(buf, 0, buf.nbytes)
            else:
                raw = np.zeros(C * rstride, dtype=np.uint8)
                for ci, h in enumerate(host):
                    for k, n, d, o in zip(names, plan.sizes, cts, roffs):
                        if h and h.get(k) is not None:
                            raw[ci * rstride + o:ci * rstride + o + n * d.itemsize] = np.ascontiguousarray(h[k], dtype=d).reshape(-1).view(np.uint8)
                buf.upload(raw)
            rem = (buf, names, plan.sizes, cts, rstride)
            self._fallback = None
        keep, srcs = [], []
        for row in rows:
            ptrs, held = _stage_host_layers(eng, [x for x, _code in row])
            srcs.append(ptrs)
            keep += held
        dts = [[code for _x, code in row] for row in rows]
        loc, vals, packed = eng.alloc(max(4 * C * lstride, 16)), eng.alloc(max(C * vstride, 16)), eng.alloc(max(8 * C * n_limbs, 16))
        table = [(plan.starts[li], TENSOR_F64 if plan.f64[li] else TENSOR_F32) for li in range(L)]
        eng.sparsify_cohort_tensors_dev(plan.total, table, plan.ks, srcs, dts, rem[0], rstride, loc, lstride, vals, vstride, packed, n_limbs, bits)
        eng.hold(keep)
        self._remain = rem
        pk = packed.download(np.uint64, C * n_limbs)          # the C packed location integers: the one download of the step
        encoded = [(int.from_bytes(pk[ci * n_limbs:(ci + 1) * n_limbs].tobytes(), "little"), K, bits, plan.total) for ci in range(C)]
        self._own_lists = [(DeviceBufferView(loc, 4 * ci * lstride, max(4 * K, 4)), K) for ci in range(C)]
        compact = [{k: CompactLayer(eng, vals, ci * vstride + o, kl, d) for k, kl, d, o in zip(names, plan.ks, cts, voffs)} for ci in range(C)]
        self._compact = ([[(cl[k].ptr, TENSOR_F64 if d == np.float64 else TENSOR_F32, d) for k, d in zip(names, cts)] for cl in compact], [vals],
                         names, [all(isinstance(x, np.ndarray) for x, _c in row) for row in rows], compact)
        self._lists = None
        return SparseCohortEncoding(encoded, list(self._own_lists), compact)

    def _sparsify_per_client(self, weights_list, walking_order, plan):
        """Every client through its own Sparsifier on the cohort's engine; the residuals move there."""
        from ._lib import TENSOR_F32, TENSOR_F64
        from .weights import CompactLayer, Sparsifier, from_big_int
        eng = self.engine
        if self._fallback is None:
            self._fallback = []
            for ci in range(self.n_local):
                sp = Sparsifier(self.sparsity, device=self.lead._device)
                sp._engine = lambda eng=eng: eng
                old = self.remain_weights(ci) if self._remain is not None else None
                if old:
                    sp.remain_weights = old
                self._fallback.append(sp)
            self._remain = None
        encoded, lists, compact, srcs, all_host = [], [], [], [], []
        for ci, (w, sp) in enumerate(zip(weights_list, self._fallback)):
            _o, layers = _client_layers(w, walking_order)
            d = {k: layers[k] for k in plan.names}
            enc = sp.sparsify(d, plan.names)
            encoded.append(enc)
            if isinstance(d[plan.names[0]], CompactLayer):
                lists.append(sp.locations)
            else:
                lists.append((eng.upload(np.asarray(from_big_int(enc[0], enc[1], enc[2], as_object=False)).astype(np.uint32)), enc[1]))
            compact.append(d)
            all_host.append(not isinstance(d[plan.names[0]], CompactLayer))
            srcs.append(None)
        self._own_lists = lists
        self._compact = (srcs, [], plan.names, all_host, compact)
        self._lists = None
        return SparseCohortEncoding(encoded, list(lists), compact)

    def remain_weights(self, c):
        """Client c's residuals {layer name: array} (what the reference keeps in Client.remain_weights), downloaded."""
        from .weights import _compact_layout
        if self._fallback is not None:
            return self._fallback[c].remain_weights
        if self._remain is None:
            return None
        buf, names, sizes, cts, stride = self._remain
        offs, nbytes = _compact_layout(sizes, cts)
        raw = buf.download_at(c * stride, np.uint8, nbytes)
        return {name: raw[o:o + n * d.itemsize].view(d).copy() for name, n, d, o in zip(names, sizes, cts, offs)}

    # ---- the arbiter's hint ----------------------------------------------------------------------------------------------------
    def dynamic_masking(self, choice=None, masks=None, total=None):
        """Without arguments the cohort IS the federation: dynamic_masking_choice over its own device lists (the arbiter's rule,
        jzf_flashe_block.py:92-112, counted on the device), then what every client's dynamic_masking(choice, masks) and cipher.total =
        total leave.  Otherwise the arbiter's answer: `masks` = the num_clients location lists of the round (host integers, DeviceBuffers
        of uint32 or (DeviceBuffer, length) pairs); after a sparsify the cohort's own clients keep the device lists it produced.
        Returns the choice."""
        from .engine import DeviceBuffer
        eng, ld = self.engine, self.lead
        if total is None:
            if self.plan is None:
                raise ValueError("dynamic_masking needs `total` (no sparsify has told the cohort the model's size)")
            total = self.plan.total
        total = int(total)
        if choice is None:
            if self.n_local != self.num_clients:
                raise ValueError(f"the cohort holds {self.n_local} of {self.num_clients} clients: dynamic_masking() needs the arbiter's choice and lists")
            if self._own_lists is None:
                raise ValueError("dynamic_masking() without arguments needs the lists of this round (sparsify first)")
            lists, sorted_all = list(self._own_lists), True
            choice = dynamic_masking_choice(lists, total, eng)
        else:
            if masks is None or len(masks) != self.num_clients:
                raise ValueError(f"masks: one location list per client of the federation ({self.num_clients})")
            lists, sorted_all = [], True
            for c, m in enumerate(masks):
                own = c - self.first_idx
                if self._own_lists is not None and 0 <= own < self.n_local:
                    lists.append(self._own_lists[own])
                elif isinstance(m, tuple):
                    lists.append((m[0], int(m[1])))
                elif isinstance(m, DeviceBuffer):
                    lists.append((m, m.nbytes // 4))
                else:
                    la = np.asarray(m, dtype=np.int64).reshape(-1)
                    if la.size and (int(la.max()) >= total or int(la.min()) < 0):
                        bad = int(la.max()) if int(la.max()) >= total else int(la.min())
                        raise IndexError(f"index {bad} is out of bounds for axis 0 with size {total}")
                    sorted_all = sorted_all and bool(np.all(la[1:] > la[:-1]))
                    lists.append((eng.upload(la.astype(np.uint32)) if la.size else eng.alloc(16), int(la.size)))
        for cl in (self._clients or [ld]):
            cl.cipher.masking_scheme = choice
            cl.cipher.masks = lists
            cl.cipher.total = total
        self._lists, self._sorted, self._host_masks = lists, sorted_all, None
        return choice

    def _host_lists(self):
        """The round's lists as host integers (what the per-client form hands to FlasheClient.dynamic_masking)."""
        if self._host_masks is None:
            self._host_masks = [buf.download_at(0, np.uint32, k).astype(np.int64) if k else np.zeros(0, dtype=np.int64) for buf, k in self._lists]
        return self._host_masks

    # ---- Client.secure_aggregate's quantise + encrypt, and the arbiter's expand + reduce --------------------------------------------
    def quantize_encrypt(self, normalize=False, seeds=None, compact=None, rng=None):
        """rng (new): the draws come from the caller's np.random.Generator (one: the clients draw one after the other, K + 1 each, the last
        one a client's 'zzz' draw) or a list of one Generator per client, as FlasheCohort.quantize_encrypt takes them: np.random.random(k)
        replaced by the generator's .random(k) on every path, the global stream untouched, Philox and PCG64-family generators on the device in ONE launch per kind.
        rng with seeds or a list of another length: ValueError; not a Generator: TypeError.

        -> SparseCohortUpload.  Client c's upload is its own FlasheClient.quantize_encrypt(compact_c + 'zzz', device=True,
        normalize=...) (K + 1 elements of uint64 limbs), `aggregate` is aggregate_sparse_uploads of the cohort's uploads.  compact: C
        dicts / Weights of compact layers given directly (host arrays, tensors or CompactLayers, with or without the trailing 'zzz'
        value; a bare list holds the compact layers in walking order) instead of the ones the last sparsify left.  seeds=None: the draws come from NumPy's global stream in client order -- client
        c takes [c (K + 1), (c + 1)(K + 1)), the last one is its 'zzz' draw -- and the generator is left where the sequential steps leave
        it; seeds=[s_0 ..]: client c draws after np.random.seed(s_c).  Generated on the device under quantize_encrypt's rule (MT19937,
        DEVICE_RNG_MIN)."""
        from .engine import DeviceVector
        ld = self.lead
        q, c = ld.quantizer, ld.cipher
        eng, C = c.engine, self.n_local
        if self._lists is None:
            raise ValueError("quantize_encrypt needs the round's masking choice and lists (dynamic_masking first)")
        if seeds is not None and len(seeds) != C:
            raise ValueError(f"seeds: one per client ({C}), got {len(seeds)}")
        if rng is not None and seeds is not None:
            raise ValueError("rng and seeds: one source of draws at a time")
        rng = _check_rng(rng, C)
        zzzs = [np.array([0.0])] * C
        if compact is not None:
            names, rows, all_host, per_client_layers = self._given_compact(compact, zzzs)
            ks, keep = [r[3] for r in rows[0]], []
            mixed = any(r[2] != r0[2] for row in rows for r, r0 in zip(row, rows[0]))
        else:
            if self._compact is None:
                raise ValueError("quantize_encrypt needs compact layers: sparsify first, or pass compact=")
            srcs0, keep0, names, all_host, per_client_layers = self._compact
            ks, keep = list(self.plan.ks), list(keep0)
            mixed = self.plan.path == PER_CLIENT
            rows = None if mixed else [[(ptr, code, d, kl) for (ptr, code, d), kl in zip(row, ks)] for row in srcs0]
        K, L = sum(ks), len(names)
        for ci in range(C):
            if self._lists[self.first_idx + ci][1] != K:
                raise ValueError(f"client {ci}: {self._lists[self.first_idx + ci][1]} locations for {K} compact values")
        zdt = {np.asarray(z).dtype for z in zzzs}
        path, _reason = _sparse_path(c.masking_scheme, bool(ld.batch), bool(ld.precompute or c.next_iter_encrypt_prepared), bool(ld.fuse),
                                     mixed or len(zdt) != 1)
        self._last = None
        if path == PER_CLIENT:
            return self._per_client(per_client_layers, names, zzzs, all_host, normalize, seeds, rng)
        # one quantiser state: the compact layers and the one-value 'zzz' layer are the layer_size_list, the lists hold the L compact layers
        alphas = _round_alphas(q, list(ks) + [1])
        q.r_max_list = [alphas[li] * q.num_clients for li in range(L)]
        q.alpha_list = [alphas[li] for li in range(L)]
        c.set_idx_list(mode="encrypt")
        # host layers of the compact= form go up once, client by client
        srcs = []
        for row in rows:
            ptrs, held = _stage_host_layers(eng, [r[0] for r in row])
            srcs.append(ptrs)
            keep += held
        dts = [[r[1] for r in row] for row in rows]
        table, at = [], 0
        for li in range(L):
            hdt = rows[0][li][2]
            shift, flags = _tensor_flags(hdt, alphas[li], normalize, q.past_layer_mean_list[li])
            table.append((at, None, alphas[li], shift, _lib.TENSOR_F64 if hdt == np.float64 else _lib.TENSOR_F32, flags))
            at += ks[li]
        zvals, z64 = self._zzz_values(zzzs, normalize, L)
        du = _cohort_draws(eng, C, K + 1, seeds, rng)
        ups = [DeviceVector(eng, K + 1) for _ in range(C)]
        zbuf = eng.alloc(max(8 * C, 16))
        front, ptbuf, pts = self._launch_uploads(path, K, table, srcs, dts, du, zvals, z64, ups, zbuf)
        zeros = [int(v) for v in zbuf.download(np.uint64, C)]          # the C quantised zeros: the one download of the step
        agg, bounds = self._aggregate(front, K, pts, ups, zeros)
        eng.hold(keep + [du, zbuf] + ([ptbuf] if ptbuf is not None else []))
        ld.shape_dict = {k: (kl,) for k, kl in zip(names, ks)}
        for u in ups:
            u.mark_ready()
        agg.mark_ready()
        self._last = SparseCohortUpload(ups, agg, SPARSE_COHORT, front)
        self._last_bounds = bounds if self.n_local == self.num_clients else None
        return self._last

    def _given_compact(self, compact, zzzs):
        """The compact= form: C dicts / Weights / bare lists of compact layers -> (names, per client [(source, dtype code, NumPy dtype of its
        host copy, size)], is every layer of client c a host array?, per client {name: layer}).  A client's 'zzz' value goes into zzzs."""
        C = self.n_local
        if len(compact) != C:
            raise ValueError(f"compact: one set of compact layers per client ({C}), got {len(compact)}")
        names, given = None, []
        for ci, w in enumerate(compact):
            if hasattr(w, "_weights") or isinstance(w, dict):
                order, layers = _client_layers(w)
            else:
                layers = {f"l{i:05d}": v for i, v in enumerate(w)}          # (a bare list: the compact layers in walking order)
                order = list(layers)
            layers = dict(layers)
            if "zzz" in layers:
                z = layers.pop("zzz")
                if interop.is_foreign(z):
                    raise TypeError("the sparse job's 'zzz' layer must be a host value")
                z = np.asarray(z)
                if z.size != 1:
                    raise ValueError(f"client {ci}: the 'zzz' layer holds {z.size} values, the sparsifier's holds one")
                zzzs[ci] = z
                order = [k for k in order if k != "zzz"]
            if names is None:
                names = order
            elif order != names:
                raise ValueError(f"client {ci}: the compact layers {order} are not client 0's {names}")
            given.append(layers)
        rows, all_host = [], []
        for ci, layers in enumerate(given):
            row = [_layer_source(self.engine, layers[k], f"client {ci} compact layer {k!r}")[:4] for k in names]
            if ci and [r[3] for r in row] != [r[3] for r in rows[0]]:
                raise ValueError(f"client {ci}: the compact layers have sizes {[r[3] for r in row]}, client 0's {[r[3] for r in rows[0]]}")
            rows.append(row)
            all_host.append(all(isinstance(r[0], np.ndarray) for r in row))
        return names, rows, all_host, given

    def _zzz_values(self, zzzs, normalize, L):
        """(the clients' 'zzz' values, are they quantised in float64?): the trailing layer as the host path takes it -- normalised with its
        own mean (NumPy's in-place rule), alpha 1.0, not encrypted."""
        q = self.lead.quantizer
        zvals, z64 = [], True
        for z in zzzs:
            a = np.ascontiguousarray(z).reshape(-1)
            if a.dtype not in (np.float32, np.float64):
                a = a.astype(np.float64)
            if normalize:
                shift = -q.past_layer_mean_list[L] if len(q.past_layer_mean_list) > L else 0.0
                a = (a.astype(_loop_dtype(a.dtype, shift)) + shift).astype(a.dtype)
            z64 = _loop_dtype(a.dtype, 1.0) == np.float64
            zvals.append(float(a[0]))
        return zvals, z64

    def _launch_uploads(self, path, K, table, srcs, dts, du, zvals, z64, ups, zbuf):
        """The uploads: ONE chained launch from the floats where the plan says so (int_bits 16 - 32: no plaintext vector in HBM, the launch
        count does not grow with C), else -- or when the library declines -- the quantise launch into plaintexts; the encrypts follow
        with the aggregate.  Returns (front end that ran, the plaintexts' buffer, client c's plaintext pointer)."""
        from . import cipher as _cipher_mod
        ld = self.lead
        q, c = ld.quantizer, ld.cipher
        eng, C = c.engine, self.n_local
        front, _why = _sparse_front_end(path, "", ld.int_bits, C, K)
        if self.prefer_front_end == FRONT_STAGED:
            front = FRONT_STAGED
        fused = getattr(eng, "quantize_encrypt_sparse_cohort_dev", None) if front == FRONT_FUSED else None
        if fused is not None and fused(c.iter_index, [self.first_idx + ci for ci in range(C)], K, _cipher_mod.N_JOBS, table, srcs, dts, q.element_bits,
                                       du, K + 1, zvals, z64, [u.buf for u in ups], zbuf):
            return FRONT_FUSED, None, None
        pstride = (8 * K + 15) & ~15
        ptbuf = eng.alloc(max(C * pstride, 16))
        pts = [ptbuf.ptr + ci * pstride for ci in range(C)]
        eng.quantize_cohort_dev(K, table, srcs, dts, q.element_bits, du, K + 1, zvals, z64, pts, [u.ptr + 8 * eng.limbs * K for u in ups], zbuf)
        return FRONT_STAGED, ptbuf, pts

    def _aggregate(self, front, K, pts, ups, zeros):
        """(aggregate, span bounds or None) of the cohort's uploads: the sparse aggregate of the ciphertexts the fused front end wrote, or
        the encrypts of the staged front end's plaintexts with it -- one fused launch over strictly increasing lists, which takes their
        span bounds and, when the cohort is the federation, leaves them to the decrypt."""
        from . import cipher as _cipher_mod
        from .engine import DeviceVector
        c = self.lead.cipher
        eng, C = c.engine, self.n_local
        own = self._lists[self.first_idx:self.first_idx + C]
        locs, lks = [b for b, _k in own], [k for _b, k in own]
        total = int(c.total)
        agg = DeviceVector(eng, total)
        outs, zs = [u.buf for u in ups], [[z, 0] for z in zeros]
        bounds = self._round_bounds(total, locs, lks) if self._sorted else None
        if front == FRONT_FUSED:
            if bounds is not None:
                eng.sparse_aggregate_dev(total, locs, lks, outs, zs, agg.buf, bounds=bounds)
            else:
                eng.sparse_aggregate_dev(total, locs, lks, outs, zs, agg.buf, sorted_lists=False)
        elif bounds is not None:
            eng.sparse_encrypt_aggregate_dev(c.iter_index, [self.first_idx + ci for ci in range(C)], locs, lks, pts, 1, zs, total, _cipher_mod.N_JOBS, outs,
                                             agg.buf, bounds=bounds)
        else:
            for ci in range(C):
                eng.encrypt_dev(c.iter_index, self.first_idx + ci, 0, K, _cipher_mod.N_JOBS, pts[ci], 1, ups[ci].buf)
            eng.sparse_aggregate_dev(total, locs, lks, outs, zs, agg.buf, sorted_lists=False)
        return agg, bounds

    def _round_bounds(self, total, locs, lks):
        """The span bounds of the round's lists, once: the aggregate takes them and, when the cohort is the federation, so does the decrypt.
        A handle of the same shape is recomputed (the list buffers may have been rewritten in place)."""
        shape = (total, self.n_local)
        if self._bounds is not None and self._bounds[1] == shape:
            bounds = self._bounds[0].recompute(locs, lks)
        else:
            bounds = self.engine.span_bounds(total, locs, lks)
        self._bounds = (bounds, shape)
        return bounds

    def _per_client(self, per_client_layers, names, zzzs, all_host, normalize, seeds, rng=None):
        """The clients' own FlasheClient steps one after the other on the shared quantiser state (one cipher re-indexed per client; with
        precompute: every client's own cipher), then aggregate_sparse_uploads of what they wrote.  What FlasheClient refuses is refused
        by the first client's step, before any draw is taken."""
        from .weights import CompactLayer
        ld = self.lead
        eng = self.engine
        masks = self._host_lists()
        ups = []
        try:
            for ci, layers in enumerate(per_client_layers):
                cl = self._clients[ci] if self._clients else ld
                cl.cipher.idx = self.first_idx + ci
                cl.cipher.masks = masks
                if seeds is not None:
                    np.random.seed(seeds[ci])
                d = {k: (layers[k].to_host() if all_host[ci] and isinstance(layers[k], CompactLayer) else layers[k]) for k in names}
                d["zzz"] = np.array(zzzs[ci], copy=True)
                lw = _Layers(d)
                up = cl.quantize_encrypt(lw, device=True, normalize=normalize, **_rng_kw(_client_rng(rng, ci)))
                ups.append(up._weights[up.walking_order[0]])
                ld.shape_dict = cl.shape_dict
        finally:
            ld.cipher.idx = self.first_idx
        own = self._lists[self.first_idx:self.first_idx + self.n_local]
        agg = aggregate_sparse_uploads(eng, ups, [b for b, _k in own] if self._sorted else masks[self.first_idx:self.first_idx + self.n_local],
                                       int(ld.cipher.total), device=True)
        self._last = SparseCohortUpload(ups, agg, PER_CLIENT)
        self._last_bounds = None
        return self._last

    # ---- Client.aggregate's decrypt + unquantise -------------------------------------------------------------------------------
    def decrypt_unquantize(self, aggregate=None, uploaded=None, out=None, unnormalize=False, degree=None, total_degree=None, last_round=None):
        """degree, total_degree, last_round (new): FlasheClient.decrypt_unquantize's, handed to the lead as they are (the sparse job's FRONT
        takes no degree: jzf_aggregator.py:676 precedes `weights - before` and the sparsifier there, so the multiply belongs to the delta
        the caller hands to sparsify).

        The new global model: set_idx_list(uploaded) + shape_dict = shape_dict_used_for_sparsification +
        FlasheClient.decrypt_unquantize(aggregate, out=, unnormalize=) of client first_idx (jzf_aggregator.py:881-899) -- the same floats,
        past_layer_mean_list / past_layer_std_list bit for bit.  Without an aggregate the cohort is the whole federation and its own last
        `aggregate` is decrypted, with the span bounds the upload computed; ValueError when clients outside the cohort exist."""
        from .cipher import _SparseMinus
        ld = self.lead
        c = ld.cipher
        degree, total_degree = ld._back_degrees(degree, total_degree)
        own = aggregate is None
        if own:
            if self.n_local != self.num_clients:
                raise ValueError(f"the cohort holds {self.n_local} of {self.num_clients} clients: decrypt_unquantize needs the federation's aggregate")
            if self._last is None:
                raise ValueError("decrypt_unquantize() without an aggregate needs the upload of this iteration (quantize_encrypt first)")
            aggregate = self._last.aggregate
        if self._lists is None:
            raise ValueError("decrypt_unquantize needs the round's masking choice and lists (dynamic_masking first)")
        if uploaded is None:
            uploaded = list(range(self.num_clients))
        if self.shape_dict_used_for_sparsification is None:
            raise ValueError("decrypt_unquantize needs the dense layer shapes (shape_dict_used_for_sparsification: sparsify sets it)")
        if not hasattr(aggregate, "walking_order"):
            aggregate = _Layers({next(iter(self.shape_dict_used_for_sparsification), "w"): aggregate})
        saved = ld.shape_dict
        ld.shape_dict = dict(self.shape_dict_used_for_sparsification)
        try:
            if c.masking_scheme == "single" and ld.fuse and not ld.batch:
                # set_idx_list_single's sparse branch (jzf_flashe.py:316-343) on lists that are in HBM already
                bounds = self._last_bounds if own and self._last is not None and self._last.path == SPARSE_COHORT else None
                c.next_iter_decrypt_prepared["minus"] = _SparseMinus(c.engine, c.iter_index, [b for b, _k in self._lists], [k for _b, k in self._lists],
                                                                     int(c.total), self._sorted, bounds=bounds)
            else:
                c.masks = self._host_lists()
                ld.set_idx_list(list(uploaded))
            return ld.decrypt_unquantize(aggregate, out=out, unnormalize=unnormalize, degree=degree, total_degree=total_degree, last_round=last_round)
        except Exception:
            ld.shape_dict = saved
            raise
