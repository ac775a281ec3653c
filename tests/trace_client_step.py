#!/usr/bin/env python3
"""Call trace of FlasheClient's fused client step on a recording engine (a script, not a test; the engine double is also what
tests/test_client_step_runs_host.py runs on).

usage: python tests/trace_client_step.py TREE OUT

Imports flashe_amd from the source tree TREE in this fresh process, puts RecordingEngine in place of the HIP engine (the cipher's and the
quantiser's), runs a grid of quantize_encrypt / decrypt_unquantize calls and writes one text file: every engine and buffer call in order
-- buffers as (ptr, nbytes) of a bump allocator, arrays as dtype, shape and a digest, scalars with their Python or NumPy type -- and after
each call the state it left (shape_dict, the quantiser's lists, the keys of the prepared dicts, _ctx_holds, a digest of NumPy's generator
state, the result's keys) or the exception it raised.  Nothing is computed and no device is touched: two trees whose traces are equal
hand the engine the same calls with the same arguments in the same order.  `diff` the files of two trees."""
import hashlib
import os
import sys

import numpy as np

LOG = []


def _digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha1(a.tobytes()).hexdigest()[:12]


def fmt(x):
    if x is None or isinstance(x, (bool, int, float, str)):
        return f"{type(x).__name__}:{x!r}"
    if isinstance(x, np.generic):
        return f"np.{type(x).__name__}:{x!r}"
    if isinstance(x, np.dtype):
        return f"dtype:{x}"
    if isinstance(x, np.ndarray):
        if x.dtype == object:
            return f"arr(object,{x.shape},{hashlib.sha1(repr(x.tolist()).encode()).hexdigest()[:12]})"
        return f"arr({x.dtype},{x.shape},{_digest(x)})"
    if isinstance(x, (bytes, bytearray)):
        return f"bytes({len(x)},{hashlib.sha1(bytes(x)).hexdigest()[:12]})"
    if isinstance(x, (list, tuple)):
        return ("[" if isinstance(x, list) else "(") + ", ".join(fmt(v) for v in x) + ("]" if isinstance(x, list) else ")")
    if isinstance(x, dict):
        return "{" + ", ".join(f"{k!r}: {fmt(v)}" for k, v in x.items()) + "}"
    if hasattr(x, "ptr") and hasattr(x, "nbytes"):
        return f"buf({x.ptr},{x.nbytes})"
    if hasattr(x, "buf") and hasattr(x, "elem_bytes"):
        return f"vec({x.n},{x.limbs},{x.elem_bytes},{fmt(x.buf)})"
    return f"<{type(x).__name__}>"


def rng_digest():
    st = np.random.get_state()
    return f"{st[0]}:{_digest(st[1])}:{st[2]}"


class Buf:
    """A device buffer of the double: an address range of the bump allocator; uploads are recorded, downloads give zeros."""

    def __init__(self, engine, nbytes):
        self.engine, self.nbytes, self.ptr = engine, int(nbytes), RecordingEngine._next
        RecordingEngine._next += (self.nbytes + 255) & ~255

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.engine._log("buf.upload", self, arr)
        return self

    def upload_at(self, offset, arr):
        arr = np.ascontiguousarray(arr)
        assert 0 <= offset and offset + arr.nbytes <= self.nbytes
        self.engine._log("buf.upload_at", self, offset, arr)
        return self

    def download(self, dtype=np.uint64, count=None):
        n = self.nbytes // np.dtype(dtype).itemsize if count is None else count
        self.engine._log("buf.download", self, np.dtype(dtype), count)
        return np.zeros(n, dtype=dtype)

    def download_at(self, offset, dtype, count):
        assert 0 <= offset and offset + int(count) * np.dtype(dtype).itemsize <= self.nbytes
        self.engine._log("buf.download_at", self, offset, np.dtype(dtype), count)
        return np.zeros(int(count), dtype=dtype)

    def free(self):
        pass


class FakeTensor:
    """A framework device tensor as far as the client step looks at one: the __cuda_array_interface__ protocol, a dtype name, a shape
    and an address.  RecordingEngine.foreign resolves it without reading memory."""

    def __init__(self, dtype, shape, ptr):
        self.dtype, self.shape, self.ptr = dtype, tuple(shape), int(ptr)

    @property
    def __cuda_array_interface__(self):
        typestr = {"float32": "<f4", "float64": "<f8", "float16": "<f2", "int32": "<i4", "uint64": "<u8"}.get(self.dtype, "<V2")
        return {"shape": self.shape, "typestr": typestr, "data": (self.ptr, False), "version": 3}


class RecordingEngine:
    """flashe_amd.engine.Engine's surface, recorded: every call goes to LOG (and to self.calls as (name, args, kwargs)) and nothing is
    computed.  Calls it does not know return None; the few host-array calls of the call-by-call step return zeros of the right shape;
    numpy_random_dev advances NumPy's stream by the draws the device call would take."""
    PREPARED_ENCRYPT, PREPARED_DECRYPT = 1, 2
    cu_count, stream = 2, 0
    _next, _count = 1 << 20, 0
    _h = None                    # (DeviceVector.__del__ destroys its event on a live ctx only: no calls at collection time)

    def __init__(self, key, int_bits, device=0, stream=None):
        self.int_bits, self.limbs, self.device, self.shared_stream = int(int_bits), 2 if int_bits > 64 else 1, device, bool(stream)
        self.tag = f"e{RecordingEngine._count}"
        RecordingEngine._count += 1
        self.calls, self._held, self._events = [], [], 0
        self._log("Engine", key, int_bits, device, stream)

    def _log(self, name, *a, **kw):
        self.calls.append((name, a, kw))
        LOG.append(f"{self.tag}.{name}(" + ", ".join([fmt(v) for v in a] + [f"{k}={fmt(v)}" for k, v in kw.items()]) + ")")

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def call(*a, **kw):
            self._log(name, *a, **kw)
        return call

    # ---- memory
    def alloc(self, nbytes):
        b = Buf(self, nbytes)
        self._log("alloc", nbytes, b)
        return b

    def alloc_vec(self, n, limbs=None):
        b = Buf(self, max(int(n) * (limbs or self.limbs) * 8, 16))
        self._log("alloc_vec", n, limbs, b)
        return b

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        b = Buf(self, max(arr.nbytes, 16))
        self._log("upload", arr, b)
        return b

    # ---- events and foreign arrays, as Engine does them
    def event(self):
        self._events += 1
        self._log("event", self._events)
        return self._events

    def event_query(self, ev):
        self._log("event_query", ev)
        return True

    def hold(self, keep):
        self._log("hold", [fmt(k) for k in keep])
        for ev, _keep in self._held:
            if self.event_query(ev):
                self.event_destroy(ev)
        self._held = []
        if keep:
            ev = self.event()
            self.record(ev)
            self._held.append((ev, keep))

    def foreign(self, obj, writable=False, what="array"):
        from flashe_amd import interop
        self._log("foreign", (obj.dtype, obj.shape, obj.ptr), writable=writable, what=what)
        return interop.ForeignArray(obj.ptr, obj.dtype, obj.shape, 10, self.device, keep=obj, source="cai")

    def compact_supported(self):
        return False

    # ---- answers the callers read
    def numpy_random_dev(self, n, out=None):
        self._log("numpy_random_dev", n, out=out)
        np.random.random(int(n))
        return None if out is not None else Buf(self, max(8 * int(n), 16))

    def quantize_encrypt_cohort_dev(self, *a, **kw):
        self._log("quantize_encrypt_cohort_dev", *a, **kw)
        return True

    def quantize_batch_encrypt_cohort_dev(self, *a, **kw):
        self._log("quantize_batch_encrypt_cohort_dev", *a, **kw)
        return True

    def quantize(self, x, alpha, element_bits, u):
        self._log("quantize", x, alpha, element_bits, u)
        return np.zeros(np.size(x), dtype=np.uint64)

    def unquantize(self, v, alpha, element_bits, num_clients):
        self._log("unquantize", v, alpha, element_bits, num_clients)
        return np.zeros(len(v), dtype=np.float64)

    def batch(self, vals, field_bits):
        self._log("batch", vals, field_bits)
        bs = self.int_bits // field_bits
        return np.zeros(((len(vals) + bs - 1) // bs, self.limbs), dtype=np.uint64)

    def unbatch(self, batched, field_bits):
        self._log("unbatch", batched, field_bits)
        return np.zeros(len(batched) * (self.int_bits // field_bits), dtype=np.uint64)

    def encrypt(self, it, idx, scheme, n_jobs, pt):
        self._log("encrypt", it, idx, scheme, n_jobs, pt)
        return np.zeros((len(pt), self.limbs), dtype=np.uint64)

    def decrypt(self, it, add_idx, minus_idx, n_jobs, ct):
        self._log("decrypt", it, add_idx, minus_idx, n_jobs, ct)
        return np.zeros((len(ct), self.limbs), dtype=np.uint64)


def install(monkey=None):
    """RecordingEngine in place of the HIP engine, for the cipher and for the quantiser's codec engines.  monkey: a pytest monkeypatch."""
    from flashe_amd import cipher as cm, quantize as qm
    put = monkey.setattr if monkey is not None else setattr
    put(cm.FlasheCipher, "_engine_cls", RecordingEngine)
    put(qm, "Engine", RecordingEngine)
    put(qm, "_engines", {})
    put(cm, "N_JOBS", 16)


class W:
    """The surface FlasheClient walks: walking_order and _weights."""

    def __init__(self, layers):
        self._weights = dict(layers)
        self.walking_order = sorted(self._weights.keys(), key=str)


KEY = bytes(range(32))


def make_client(int_bits, batch=False, element_bits=16, mask="double", num_params=None, num_clients=3, idx=0, it=3):
    from flashe_amd.block import FlasheClient
    args = {"quantize": {"int_bits": int_bits, "batch": batch, "element_bits": element_bits, "padding": True, "secure": True},
            "precompute": {"enable": num_params is not None, "num_params": num_params}}
    cl = FlasheClient(args)
    cl.create_cipher(idx, num_clients, KEY)
    cl.cipher.masking_scheme = mask
    cl.set_iter_index(it)
    return cl


# ------------------------------------------------------------------------------------------------------------------ the grid
N_CASES = [0]


def case(name):
    N_CASES[0] += 1
    RecordingEngine._next = 1 << 20                  # (addresses restart with every case: a difference stays inside its case)
    LOG.append(f"==== {name}")


def state(cl):
    q, c = cl.quantizer, cl.cipher
    LOG.append(f"  shape_dict={cl.shape_dict!r}")
    LOG.append(f"  alpha_list={fmt(q.alpha_list)} r_max_list={fmt(q.r_max_list)} shape_list={q.shape_list!r} layer_size_list={fmt(q.layer_size_list)}")
    LOG.append(f"  mean={fmt(q.past_layer_mean_list)} std={fmt(q.past_layer_std_list)}")
    LOG.append(f"  prepared: encrypt={sorted(c.next_iter_encrypt_prepared)} decrypt={sorted(c.next_iter_decrypt_prepared)} "
               f"decrypt_idx={sorted(c.next_iter_decrypt_prepared_idx)} prefixes={fmt(c.index_prefix_for_add)} / {fmt(c.index_prefix_for_minus)}")
    LOG.append(f"  ctx_holds={c._ctx_holds} rng={rng_digest()}")


def call(cl, what, fn):
    LOG.append(f"-- {what}")
    try:
        res = fn()
    except Exception as e:                          # every refusal, with its message
        LOG.append(f"  raised {type(e).__name__}: {e}")
        res = None
    else:
        if hasattr(res, "_weights"):
            LOG.append("  result " + ", ".join(f"{k!r}: {fmt(res._weights[k])}" for k in res.walking_order))
        else:
            LOG.append(f"  result {fmt(res)}")
    if cl is not None:
        state(cl)
    return res


def host_layers(dtype=np.float32, sizes=(4, 3, 0, 6, 2), seed=1):
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {}
    for i, s in enumerate(sizes):
        shape = (s,) if i % 2 else (s // 2, 2) if s % 2 == 0 and s else (s,)
        a = rng.standard_normal(s).reshape(shape)
        out[f"l{i}"] = (a * 100).astype(dtype) if np.issubdtype(np.dtype(dtype), np.integer) else a.astype(dtype)
    return out


def tensor_layers(dtypes, sizes=(4, 3, 0, 6, 2)):
    """Fake tensors of the given dtypes in turn; None in dtypes = a host float32 layer there."""
    out, host = {}, host_layers(np.float32, sizes)
    for i, s in enumerate(sizes):
        dt = dtypes[i % len(dtypes)]
        out[f"l{i}"] = host[f"l{i}"] if dt is None else FakeTensor(dt, (s,), 0x7000_0000 + 4096 * i)
    return out


WIDTHS = [dict(int_bits=128), dict(int_bits=120, batch=True), dict(int_bits=64), dict(int_bits=20), dict(int_bits=64, batch=True, element_bits=8)]
SIZES = (4, 3, 0, 6, 2)


def _label(kw):
    return "b%d%s%s" % (kw["int_bits"], "-batched" if kw.get("batch") else "", "-e%d" % kw["element_bits"] if "element_bits" in kw else "")


def _elems(kw, sizes=SIZES, num_clients=3):
    if not kw.get("batch"):
        return sum(sizes)
    bs = kw["int_bits"] // (kw.get("element_bits", 16) + int(np.ceil(np.log2(num_clients))))
    return sum((s + bs - 1) // bs for s in sizes)


def round_trip(name, kw, mask="double", prepared=None, layers=None, device=True, normalize=False, fuse=True, dec_prepared=None,
               dropouts=False, unnormalize=False, out=None, aggregate="vec", run_max=None, num_params=None):
    """One quantize_encrypt and one decrypt_unquantize of the same client.  prepared / dec_prepared: None, "ctx" (the handles prepare_*
    leave), "single", "arrays" (vectors a caller assigned: call by call), "short" (a cache of another length)."""
    from flashe_amd import block
    from flashe_amd.cipher import _DevVec
    from flashe_amd.engine import DeviceVector
    case(name)
    ne = _elems(kw, [v.size if isinstance(v, np.ndarray) else int(np.prod(v.shape)) for k, v in (host_layers() if layers is None else layers).items() if k != "zzz"])
    if num_params is None and (prepared in ("ctx", "single", "short") or dec_prepared in ("ctx", "short")):
        num_params = ne + (1 if "short" in (prepared, dec_prepared) else 0)
    cl = make_client(mask=mask, num_params=num_params if prepared in ("ctx", "single", "short") or dec_prepared in ("ctx", "short") else None, **kw)
    c = cl.cipher
    if num_params is not None and prepared is None:
        c.discard_prepared_encrypt()
    if prepared == "arrays":
        c.next_iter_encrypt_prepared = {"add": _DevVec(c.engine, ne), "minus": _DevVec(c.engine, ne)}
    cl.fuse = fuse
    saved = block._RNG_RUN_MAX
    if run_max is not None:
        block._RNG_RUN_MAX = run_max
    np.random.seed(7)
    w = W(layers if layers is not None else host_layers())
    try:
        res = call(cl, f"quantize_encrypt(device={device}, normalize={normalize})", lambda: cl.quantize_encrypt(w, device=device, normalize=normalize))
    finally:
        block._RNG_RUN_MAX = saved
    if res is None:
        return cl
    k0 = res.walking_order[0] if res.walking_order else None
    if k0 is None:
        return cl
    n = len(res._weights[k0])
    if dec_prepared in ("ctx", "short"):
        call(cl, "prepare_decrypt", lambda: cl.prepare_decrypt())
    elif dec_prepared == "arrays":
        c.next_iter_decrypt_prepared = {"add": _DevVec(c.engine, n), "minus": _DevVec(c.engine, n)}
    call(cl, "set_idx_list", lambda: cl.set_idx_list([0, 2] if dropouts else [0, 1, 2]))
    if dec_prepared == "single":
        c.next_iter_decrypt_prepared["minus"] = _DevVec(c.engine, n)
    if aggregate == "vec":
        agg = DeviceVector(c.engine, n)
    elif aggregate == "limbs":
        agg = np.arange(n * c.engine.limbs, dtype=np.uint64).reshape(n, c.engine.limbs)
    elif aggregate == "ints":
        agg = np.array([int(v) for v in range(n)], dtype=object)
    else:
        agg = FakeTensor("uint64", (n, c.engine.limbs) if c.engine.limbs == 2 else (n,), 0x6000_0000)
    outs = None
    if out is not None:
        shapes = cl.quantizer.shape_list if cl.batch else list(cl.shape_dict.values())
        outs = {k: FakeTensor(out[i % len(out)], shp, 0x5000_0000 + 4096 * i) for i, (k, shp) in enumerate(zip(cl.shape_dict, shapes))}
    call(cl, f"decrypt_unquantize(out={out}, unnormalize={unnormalize}, aggregate={aggregate})",
         lambda: cl.decrypt_unquantize(W({k0: agg}), out=outs, unnormalize=unnormalize))
    return cl


def sparse_cases():
    from flashe_amd.engine import DeviceVector
    for kw in (dict(int_bits=128), dict(int_bits=20)):
        for mask in ("single", "double"):
            for tensors in (False, True):
                for normalize in (False, True):
                    case(f"sparse job {_label(kw)} {mask} tensors={tensors} normalize={normalize}")
                    cl = make_client(mask=mask, **kw)
                    layers = tensor_layers(["float32", None, "float64", "float16"]) if tensors else host_layers()
                    layers["zzz"] = np.array([0.25], dtype=np.float32)
                    np.random.seed(9)
                    res = call(cl, "quantize_encrypt", lambda: cl.quantize_encrypt(W(layers), normalize=normalize))
                    # the arbiter's dense aggregate comes back: location masks on the cipher, the dense shapes in shape_dict
                    c = cl.cipher
                    c.masks, c.total = [[0, 2, 5], [1, 2, 7]], 9
                    cl.shape_dict = {"l0": (2, 2), "l1": (5,)}
                    cl.quantizer.alpha_list = cl.quantizer.alpha_list[:2]
                    call(cl, "set_idx_list", lambda: cl.set_idx_list([0, 1, 2]))
                    call(cl, "decrypt_unquantize", lambda: cl.decrypt_unquantize(W({"l0": DeviceVector(c.engine, 9)})))
                    call(cl, "set_idx_list", lambda: cl.set_idx_list([0, 1, 2]))
                    outs = {"l0": FakeTensor("float32", (2, 2), 0x5000_0000), "l1": FakeTensor("float64", (5,), 0x5000_1000)}
                    call(cl, "decrypt_unquantize(out=)", lambda: cl.decrypt_unquantize(W({"l0": DeviceVector(c.engine, 9)}), out=outs, unnormalize=normalize))
                    call(cl, "set_idx_list", lambda: cl.set_idx_list([0, 1, 2]))
                    cl.shape_dict = {"l0": (2, 2), "l1": (6,)}                                   # describes more than the aggregate holds
                    call(cl, "decrypt_unquantize(too long)", lambda: cl.decrypt_unquantize(W({"l0": DeviceVector(c.engine, 9)})))
                    call(cl, "set_idx_list", lambda: cl.set_idx_list([0, 1, 2]))
                    call(cl, "decrypt_unquantize(out=, too long)",
                         lambda: cl.decrypt_unquantize(W({"l0": DeviceVector(c.engine, 9)}), out={"l0": outs["l0"], "l1": FakeTensor("float64", (6,), 0x5000_1000)}))


def refusal_cases():
    from flashe_amd.engine import DeviceVector
    t = lambda: tensor_layers(["float32"])
    for name, setup, layers in [
            ("tensors: fuse=False", lambda cl: setattr(cl, "fuse", False), t()),
            ("tensors: location masks", lambda cl: setattr(cl.cipher, "masks", [[0]]), t()),
            ("tensors: unsupported dtype", lambda cl: None, tensor_layers(["int32"])),
            ("tensors sparse: fuse=False", lambda cl: setattr(cl, "fuse", False), dict(t(), zzz=np.array([0.5]))),
            ("tensors sparse: zzz not last", lambda cl: None, {"zzz": np.array([0.5]), "zzzz": FakeTensor("float32", (3,), 0x7000_0000)}),
            ("tensors sparse: zzz foreign", lambda cl: None, dict(t(), zzz=FakeTensor("float32", (1,), 0x7100_0000))),
            ("tensors sparse: zzz of two values", lambda cl: None, dict(t(), zzz=np.array([0.5, 0.5])))]:
        case("refusal " + name)
        cl = make_client(128)
        setup(cl)
        call(cl, "quantize_encrypt", lambda: cl.quantize_encrypt(W(layers)))
    for name, kw in [("tensors sparse: batched", dict(int_bits=120, batch=True)), ("tensors sparse: cache", dict(int_bits=128, num_params=15))]:
        case("refusal " + name)
        cl = make_client(**kw)
        call(cl, "quantize_encrypt", lambda: cl.quantize_encrypt(W(dict(t(), zzz=np.array([0.5])))))
    case("host sparse: batched and cache go call by call")
    for kw in (dict(int_bits=120, batch=True), dict(int_bits=128, num_params=15)):
        cl = make_client(**kw)
        np.random.seed(5)
        call(cl, "quantize_encrypt", lambda: cl.quantize_encrypt(W(dict(host_layers(), zzz=np.array([0.5])))))
    # the decrypt side
    for name, setup, kwargs in [
            ("out=: zzz in the upload", lambda cl, w: w._weights.update(zzz=np.zeros(1)), {}),
            ("out=: fuse=False", lambda cl, w: setattr(cl, "fuse", False), {}),
            ("out=: no shape_dict", lambda cl, w: setattr(cl, "shape_dict", None), {}),
            ("out=: a layer missing", lambda cl, w: None, {"drop": "l1"}),
            ("out=: a host array", lambda cl, w: None, {"host": "l1"}),
            ("out=: integer tensor", lambda cl, w: None, {"dtype": "int32"}),
            ("out=: another shape", lambda cl, w: None, {"shape": (9,)}),
            ("out=: sparse double mask", lambda cl, w: setattr(cl.cipher, "masks", [[0]]), {}),
            ("out=: sparse fuse=False", lambda cl, w: (setattr(cl.cipher, "masks", [[0]]), setattr(cl, "fuse", False)), {}),
            ("out=: sparse without the location masks", lambda cl, w: (setattr(cl.cipher, "masks", [[0]]), setattr(cl.cipher, "masking_scheme", "single")), {}),
            ("out=: no prefixes", lambda cl, w: cl.cipher.set_idx_list(mode="encrypt") or setattr(cl.cipher, "index_prefix_for_add", None) or
             setattr(cl.cipher, "index_prefix_for_minus", None), {}),
            ("out=: shape_dict describes more than the aggregate", lambda cl, w: cl.shape_dict.update(l4=(40,)), {"shape4": (40,)})]:
        case("refusal " + name)
        cl = make_client(128)
        np.random.seed(5)
        res = cl.quantize_encrypt(W(host_layers()))
        cl.set_idx_list([0, 1, 2])
        w = W({"l0": res._weights["l0"]})
        outs = {k: FakeTensor(kwargs.get("dtype", "float32"), kwargs.get("shape", shp) if k == "l1" else shp, 0x5000_0000 + 4096 * i)
                for i, (k, shp) in enumerate(cl.shape_dict.items())}
        setup(cl, w)
        if "shape4" in kwargs:
            outs["l4"] = FakeTensor("float32", kwargs["shape4"], 0x5000_4000)
        if "drop" in kwargs:
            del outs[kwargs["drop"]]
        if "host" in kwargs:
            outs[kwargs["host"]] = np.zeros(3)
        LOG.append("-- (encrypt and set_idx_list above)")
        call(cl, "decrypt_unquantize(out=)", lambda: cl.decrypt_unquantize(w, out=outs))
    case("refusal out=: batched sparse")
    cl = make_client(120, batch=True)
    cl.cipher.masks = [[0]]
    cl.shape_dict = {"l0": (1,)}
    call(cl, "decrypt_unquantize(out=)", lambda: cl.decrypt_unquantize(W({"l0": DeviceVector(cl.cipher.engine, 1)}), out={}))
    for kw in (dict(int_bits=128), dict(int_bits=120, batch=True)):
        case(f"refusal decrypt {_label(kw)}: an aggregate of another length, no prefixes")
        cl = make_client(**kw)
        np.random.seed(5)
        cl.quantize_encrypt(W(host_layers()))
        cl.set_idx_list([0, 1, 2])
        call(cl, "decrypt_unquantize(short)", lambda: cl.decrypt_unquantize(W({"l0": DeviceVector(cl.cipher.engine, 2)})))
        cl.cipher.index_prefix_for_add, cl.cipher.index_prefix_for_minus = [], []
        call(cl, "decrypt_unquantize(no prefixes)", lambda: cl.decrypt_unquantize(W({"l0": DeviceVector(cl.cipher.engine, _elems(kw))})))


def cohort_lead_cases():
    """_CohortLead._decrypt_floats as tests/test_cohort_batch_planner.py drives it, batched and not."""
    from flashe_amd.block import FlasheCohort, cohort_admission_length
    from flashe_amd.engine import DeviceVector
    adm = cohort_admission_length(RecordingEngine.cu_count)
    for b, batch in ((120, True), (128, False)):
        case(f"cohort lead b{b} batched={batch}")
        args = {"quantize": {"int_bits": b, "batch": batch, "element_bits": 16, "padding": True, "secure": True}, "precompute": {"enable": False}}
        co = FlasheCohort(args, first_idx=0, n_local=3, num_clients=3, prp_seed=KEY)
        co.set_iter_index(4)
        sizes = [7, 0, (6 if batch else 1) * (adm - 2) + 5]
        np.random.seed(3)
        up = call(co.lead, "cohort.quantize_encrypt", lambda: co.quantize_encrypt([W({f"l{i}": np.zeros(s, np.float32) for i, s in enumerate(sizes)}) for _ in range(3)]))
        ld = co.lead
        LOG.append(f"  path={up.path} mask={ld._cohort_mask is not None}")
        n = len(up.partial_sum)
        for what, dv, szs, add, minus, it in [("the sum", up.partial_sum, sizes, [3], [0], 4), ("another vector", DeviceVector(ld.cipher.engine, n), sizes, [3], [0], 4),
                                              ("another iteration", up.partial_sum, sizes, [3], [0], 5), ("other clients", up.partial_sum, sizes, [2], [0], 4),
                                              ("too many values", up.partial_sum, [sizes[0], sizes[1], sizes[2] + 6 * n], [3], [0], 4)]:
            ld.cipher.set_iter_index(it)
            call(ld, f"_decrypt_floats({what})", lambda: ld._decrypt_floats(dv, szs, None, add, minus))
        call(ld, "cohort.decrypt_unquantize", lambda: co.decrypt_unquantize())


def grid():
    for kw in WIDTHS:
        lb = _label(kw)
        for mask in ("double", "single"):
            round_trip(f"{lb} {mask} online", kw, mask=mask)
            round_trip(f"{lb} {mask} prepared ctx", kw, mask=mask, prepared="ctx" if mask == "double" else "single", dec_prepared="ctx" if mask == "double" else "single")
            round_trip(f"{lb} {mask} tensors", kw, mask=mask, layers=tensor_layers(["float32", "float64", None, "float16", "bfloat16"]), out=["float32", "float64", "float16", "bfloat16"])
        round_trip(f"{lb} prepared ctx, dropouts", kw, prepared="ctx", dec_prepared="ctx", dropouts=True)
        round_trip(f"{lb} online, dropouts", kw, dropouts=True)
        round_trip(f"{lb} prepared arrays: call by call", kw, prepared="arrays", dec_prepared="arrays")
        round_trip(f"{lb} prepared cache of another length", kw, prepared="short")
        round_trip(f"{lb} decrypt cache of another length", kw, dec_prepared="short")
        round_trip(f"{lb} tensors, prepared ctx, normalize", kw, prepared="ctx", dec_prepared="ctx", normalize=True, unnormalize=True,
                   layers=tensor_layers(["float32", "float64", None, "float16", "bfloat16"]), out=["float64", "float32"])
        round_trip(f"{lb} tensors, cache of another length", kw, prepared="short", layers=tensor_layers(["float32"]))
        round_trip(f"{lb} normalize / unnormalize", kw, normalize=True, unnormalize=True)
        round_trip(f"{lb} device=False", kw, device=False, aggregate="limbs")
        round_trip(f"{lb} fuse=False", kw, fuse=False, aggregate="ints")
        for dt in (np.float64, np.int32):
            round_trip(f"{lb} host {np.dtype(dt)}", kw, layers=host_layers(dt))
        round_trip(f"{lb} host mixed, 0-d and empty", kw, layers={"a": np.float32(0.5), "b": np.zeros((0, 3), np.float64), "c": np.arange(5), "d": np.ones(3, np.float32)})
        round_trip(f"{lb} empty model", kw, layers={})
        round_trip(f"{lb} empty model, prepared ctx", kw, layers={}, prepared="ctx")
        round_trip(f"{lb} only empty layers", kw, layers={"a": np.zeros(0, np.float32), "b": np.zeros((0, 2))})
        round_trip(f"{lb} only empty tensors, prepared ctx", kw, layers={"a": FakeTensor("float32", (0,), 0x7000_0000)}, prepared="ctx")
        for agg in ("limbs", "ints", "foreign"):
            round_trip(f"{lb} aggregate as {agg}", kw, aggregate=agg)
            round_trip(f"{lb} aggregate as {agg}, out=", kw, aggregate=agg, out=["float32"])
        round_trip(f"{lb} out= and unnormalize", kw, out=["float64", "float16"], unnormalize=True)
        for prep in (None, "ctx"):
            round_trip(f"{lb} run length 5, prepared={prep}", kw, run_max=5, prepared=prep)
            round_trip(f"{lb} run length 5, tensors, prepared={prep}", kw, run_max=5, prepared=prep, layers=tensor_layers(["float32", "float64", None]))
    round_trip("b128 a layer large enough for the device draws", dict(int_bits=128), layers={"a": np.zeros(3, np.float32), "b": np.zeros(70000, np.float32)})
    round_trip("b120-batched a model large enough for the device draws", dict(int_bits=120, batch=True), layers={"a": np.zeros(70000, np.float32)})
    sparse_cases()
    refusal_cases()
    cohort_lead_cases()


def main():
    tree, out = os.path.abspath(sys.argv[1]), sys.argv[2]
    sys.path[:] = [tree] + [p for p in sys.path if os.path.abspath(p or ".") not in (tree, os.path.dirname(os.path.abspath(__file__)))]
    import flashe_amd
    assert os.path.abspath(flashe_amd.__file__).startswith(tree + os.sep), flashe_amd.__file__
    install()
    grid()
    with open(out, "w") as f:
        f.write("\n".join(LOG) + "\n")
    print(f"{N_CASES[0]} cases, {len(LOG)} lines -> {out}")


if __name__ == "__main__":
    main()
