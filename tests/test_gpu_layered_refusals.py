"""GPU: the refusals of the entry points that take a per-layer table (flashe_amd/csrc/abi_layers.hip): the model-wide and batched
codec, the tensor forms, the prepared client step, the dense, prepared and sparse cohorts, the layer-wise sparsifier and
flashe_store_layers_dev.

Every case is a valid call with ONE bad argument, so no precedence between checks can matter; it asserts the code (FLASHE_EINVAL), a
substring of the message, and that every output buffer still holds its poison pattern.  The calls go through the ctypes handle that
Engine itself uses (Engine._lib / Engine._h): Engine's wrappers build the tables and their counts from Python lists, so a null table, a
non-zero reserved field or a count that disagrees with the table cannot be said through them, and one driver for every entry point
keeps each case at exactly one fault.  The arguments Engine does pass through are checked through it as well (test_through_engine).

Shapes: a model of n = 13 values in three layers of 5, 0 and 8 (starts 0, 5, 5: the empty layer takes the start == end skip), engines at
int_bits 128 (two limbs, 16-byte vectors), 20 and -- the one-limb cohort -- 40 (one limb), the batched form at 128 with element_bits 16 in fields of 24 bits (5 values
per element: 1 + 0 + 2 = 3 elements), cohorts of 2 clients.  The dense cohorts -- all twelve forms of the chained launch: first_idx or an
index list, wide, compact, one-limb or batched, whole or cut -- check their sources and alphas only once the launch has admitted the shape, so those
cases run at the smallest size it admits on one compute unit (the cut forms: n = 13 as it is).  The prepared cohorts -- all eight forms of
the online launch: a draw buffer or a Philox / PCG64 segment table, wide, compact or batched -- have no admission, so every case runs at
n = 13; a form that draws inside the launch is given ONE segment tiling the clients' 2 n values, and every refusal leaves it as it was.
"""
import copy
import ctypes
import math

import numpy as np
import pytest

from flashe_amd import Engine, _lib
from flashe_amd._lib import FlasheError

pytestmark = pytest.mark.gpu

EINVAL, ENOTSUP, OK = -22, _lib.ENOTSUP, 0
KEY = bytes(range(32))
N, STARTS, SIZES = 13, (0, 5, 5), (5, 0, 8)
EB, FB = 16, 24
POISON = 0xA5
F32, F64, F16 = _lib.TENSOR_F32, _lib.TENSOR_F64, _lib.TENSOR_F16
c_vp = ctypes.c_void_p

NV, A16, A8, MV = "null vector", "2-limb elements must be 16-byte aligned", "device vectors must be 8-byte aligned", "misaligned vector"
U8, O8 = "u_dev must be 8-byte aligned", "out_dev must be 8-byte aligned"
TABLE, START0, ASCEND = "the layer table needs at least one entry", "layers[0].start must be 0", "starts must ascend and stay within n"
BITS_FRONT, BITS_BACK, BITS_BATCH = "element_bits must be in [1, min(62, int_bits)]", "element_bits must be in [1, 62]", \
    "need 1 <= element_bits <= field_bits <= int_bits"
COUNT, RANGE, NCL = "the layers batch into", "exceeds n", "num_clients must be >= 1"
ALPHA = "alpha must be positive"


# ---- ctypes marshalling: one spec string per entry point, "name" or "name:kind" in the order of include/flashe.h ----
def _layers(kind, rows):
    if rows is None:
        return None
    if kind in "CB":
        arr = (_lib.CodecLayer if kind == "C" else _lib.BatchLayer) * max(len(rows), 1)
        arr = arr()
        for i, (a, x, alpha, f64, res) in enumerate(rows):
            if kind == "C":
                arr[i].start = a
            else:
                arr[i].size = a
            arr[i].x_dev, arr[i].alpha, arr[i].x_is_f64, arr[i].reserved = x, alpha, f64, res
        return arr
    arr = (_lib.TensorLayer * max(len(rows), 1))()
    for i, (start, ptr, alpha, shift, dtype, flags) in enumerate(rows):
        arr[i].start, arr[i].ptr, arr[i].alpha, arr[i].shift, arr[i].dtype, arr[i].flags = start, ptr, alpha, shift, dtype, flags
    return arr


_ARRAYS = {"U32": ctypes.c_uint32, "U64": ctypes.c_uint64, "I32": ctypes.c_int32, "D": ctypes.c_double, "P": c_vp}
_SEGMENTS = {"PX": _lib.PhiloxSegment, "PG": _lib.Pcg64Segment}          # a segment table: one dict of fields per segment, tuples for the arrays


def _marshal(kind, v):
    if v is None:
        return None
    if kind in ("C", "B", "T"):
        return _layers(kind, v)
    if kind in _ARRAYS:
        return (_ARRAYS[kind] * max(len(v), 1))(*v)
    if kind in _SEGMENTS:
        arr = (_SEGMENTS[kind] * max(len(v), 1))()
        for seg, fields in zip(arr, v):
            for field, value in fields.items():
                setattr(seg, field, type(getattr(seg, field))(*value) if isinstance(value, tuple) else value)
        return arr
    return v


class EP:
    """One entry point: its C name, argument spec, the int_bits it is driven at, the code a valid call returns and its case list."""

    def __init__(self, name, spec, table, widths=(128, 20), ok=OK, prep=None, cohort=False):
        self.name, self.table, self.widths, self.ok, self.prep, self.cohort = name, table, widths, ok, prep, cohort
        self.args = [(s.split(":") + [""])[:2] for s in spec.split()]

    def call(self, r, a):
        fn = getattr(r.lib, "flashe_" + self.name)
        keep = [_marshal(kind, a[name]) for name, kind in self.args]
        r.kept = {name: v for (name, _kind), v in zip(self.args, keep)}       # (what the call was given, as the call left it)
        rc = fn(r.h, *keep)
        msg = r.lib.flashe_last_error(r.h)
        return rc, (msg.decode() if msg else "")


class Rig:
    """An engine with the sources, inputs and poisoned outputs of every entry point at the module's shapes."""

    def __init__(self, bits, n=N, starts=STARTS):
        self.bits, self.n = bits, n
        self.eng = Engine(KEY, bits)
        self.lib, self.h, self.L = self.eng._lib, self.eng._h, self.eng.limbs
        self.starts = starts
        self.sizes = [(starts[l + 1] if l + 1 < len(starts) else n) - starts[l] for l in range(len(starts))]
        rng = np.random.Generator(np.random.PCG64(bits))
        L, vb = self.L, n * self.L * 8
        self.bs = bits // FB if bits >= FB else 1
        self.n_elems = sum((s + self.bs - 1) // self.bs for s in self.sizes)
        self.ins, self.outs = {}, {}

        def inp(name, arr):
            self.ins[name] = self.eng.alloc(arr.nbytes + 32).upload(arr)
            return self.ins[name].ptr

        def out(name, nbytes):
            self.outs[name] = self.eng.alloc(nbytes + 32)
            return self.outs[name].ptr

        self.x = [inp("x%d" % c, (0.1 * rng.standard_normal(n)).astype(np.float32)) for c in range(2)]
        self.h16 = inp("h16", (0.1 * rng.standard_normal(n)).astype(np.float16))
        self.u = inp("u", rng.random(2 * (n + 1)))
        mask = (1 << min(bits, 64)) - 1
        for name in ("vin", "add", "minus"):
            setattr(self, name, inp(name, rng.integers(0, 2 ** 63, n * L, dtype=np.uint64) & np.uint64(mask)))
        self.mask = [inp("mask%d" % c, rng.integers(0, 2 ** 63, n * L, dtype=np.uint64) & np.uint64(mask)) for c in range(2)]
        self.ct = [out("ct%d" % c, vb + 8) for c in range(2)]
        self.sum, self.dmask, self.fout = out("sum", vb), out("dmask", vb), out("fout", n * 8)
        self.store, self.stats = out("store", n * 4), out("stats", 2 * len(starts) * 8)
        self.residual, self.loc, self.vals, self.packed = out("residual", 256), out("loc", 256), out("vals", 256), out("packed", 256)
        self.pt = [out("pt%d" % c, (n + 1) * 8) for c in range(2)]
        self.tail = [out("tail%d" % c, 16) for c in range(2)]
        self.zeros = out("zeros", 16)
        self.scratch = out("scratch", 4 * vb)                              # (a cut launch's: two pieces' sums and masks would fit)
        self.poison()

    def poison(self):
        for b in self.outs.values():
            self.eng.memset_dev(b, POISON, b.nbytes)
        self.eng.sync()

    def snapshot(self):
        self.eng.sync()
        return {k: b.download(np.uint8).copy() for k, b in self.outs.items()}

    def dirty(self):
        return [k for k, v in self.snapshot().items() if not (v == POISON).all()]

    def layer_ptrs(self, base, es):
        return [base + s * es for s in self.starts]

    # the valid call of every entry point
    def defaults(self, ep):
        n, x = self.n, self.layer_ptrs(self.x[0], 4)
        C = [[s, p, 1.0, 0, 0] for s, p in zip(self.starts, x)]
        B = [[s, p, 1.0, 0, 0] for s, p in zip(self.sizes, x)]
        # layer 0 in float16 (it goes through the stage pass), the others float32 read in place
        T = [[s, p, 1.0, 0.0, F32, 0] for s, p in zip(self.starts, x)]
        T[0][1], T[0][4] = self.h16, F16
        S = [[s, None, 1.0, 0.0, F32, 0] for s in self.starts]
        st = self.layer_ptrs(self.store, 4)
        a = dict(iter=3, idx=0, scheme=1, n=n, n_values=n, n_jobs=1, first=0, count=n, eb=EB, fb=FB, u=self.u, ct=self.ct[0], out=self.fout,
                 fout=self.fout, vin=self.vin, add=[1], n_add=1, minus=[0], n_minus=1, padd=[], n_padd=0, pminus=[], n_pminus=0, nc=2,
                 vadd=self.add, vminus=self.minus, n_elems=self.n_elems, layers=C, n_layers=len(self.starts), block=4, stats=self.stats,
                 k=[2, 0, 3], residual=self.residual, loc=self.loc, vals=self.vals, packed=self.packed, pbits=8, first_idx=0, n_clients=2,
                 src=[p for c in range(2) for p in self.layer_ptrs(self.x[c], 4)], sdt=[F32] * (2 * len(self.starts)), cts=list(self.ct),
                 sum=self.sum, dmask=self.dmask, rstride=64, lstride=8, vstride=24, pstride=1, u_stride=n + 1, zzz=[0.5, 0.25], zf64=1,
                 pts=list(self.pt), tails=list(self.tail), zeros=self.zeros, cidx=[0, 1], scratch=self.scratch, masks=list(self.mask), n_segs=1)
        if "philox" in ep.name:
            a["segs"] = [dict(key=(1, 2), counter=(3, 4, 5, 6), buffer=(7, 8, 9, 10), buffer_pos=2, n=2 * n, offset=0)]
        if "pcg64" in ep.name:
            a["segs"] = [dict(state=(11, 12), inc=(13, 14), variant=0, n=2 * n, offset=0)]
        a["layers"] = copy.deepcopy({"C": C, "B": B, "T": T, "S": S}[ep.table])
        if ep.name == "store_layers_dev":
            for l in range(len(self.starts)):
                a["layers"][l][1], a["layers"][l][4] = st[l], F32
        if ep.name in ("quantize_cohort_dev", "quantize_encrypt_sparse_cohort_dev"):
            a["cts"] = list(self.pt)
        return a

    def prepare(self, which, n):
        """The ctx's cache of `which` holds masks of n elements (None: holds nothing)."""
        held, have, _a, _m = self.eng.prepared_query(1 if which == "enc" else 2)
        if n is None:
            self.eng.prepared_discard(1 if which == "enc" else 2)
        elif not held or have != n:
            if which == "enc":
                self.eng.prepare_encrypt(4, 0, 1, n, 1)
            else:
                self.eng.prepare_decrypt(3, 2, n, 1)

    def run(self, ep, a):
        if ep.prep:
            self.prepare(ep.prep[0], a.get("_prep", a[ep.prep[1]]))
        return ep.call(self, a)


MODEL_FRONT = "iter idx scheme n n_jobs first count layers:C n_layers eb u ct"
EPS = [
    EP("quantize_encrypt_model_dev", MODEL_FRONT, "C"),
    EP("decrypt_unquantize_model_dev", "iter add:U32 n_add minus:U32 n_minus n n_jobs first count vin layers:C n_layers eb nc fout", "C"),
    EP("unquantize_model_dev", "n first count vin layers:C n_layers eb nc fout", "C"),
    EP("combine_unquantize_model_dev", "n vin vadd vminus layers:C n_layers eb nc fout", "C"),
    EP("quantize_encrypt_prepared_model_dev", "n first count layers:C n_layers eb u ct", "C", prep=("enc", "n")),
    EP("decrypt_prepared_unquantize_model_dev", "iter padd:U32 n_padd pminus:U32 n_pminus n n_jobs vin layers:C n_layers eb nc fout", "C",
       prep=("dec", "n")),
    EP("quantize_batch_model_dev", "layers:B n_layers eb fb u n_elems ct", "B", widths=(128,)),
    EP("unbatch_unquantize_model_dev", "layers:B n_layers eb fb nc vin n_elems fout", "B", widths=(128,)),
    EP("combine_unbatch_unquantize_model_dev", "layers:B n_layers eb fb nc vin vadd vminus n_elems fout", "B", widths=(128,)),
    EP("quantize_batch_encrypt_prepared_model_dev", "layers:B n_layers eb fb u n_elems ct", "B", widths=(128,), prep=("enc", "n_elems")),
    EP("decrypt_prepared_unbatch_unquantize_model_dev", "iter padd:U32 n_padd pminus:U32 n_pminus n_jobs layers:B n_layers eb fb nc vin n_elems fout",
       "B", widths=(128,), prep=("dec", "n_elems")),
    EP("quantize_encrypt_tensors_dev", MODEL_FRONT.replace(":C", ":T"), "T"),
    EP("quantize_batch_tensors_dev", "layers:T n_layers n_values eb fb u n_elems ct", "T", widths=(128,)),
    EP("store_layers_dev", "vin n layers:T n_layers block stats", "T"),
    EP("quantize_encrypt_prepared_tensors_dev", "n first count layers:T n_layers eb u ct", "T", prep=("enc", "n")),
    EP("quantize_batch_encrypt_prepared_tensors_dev", "layers:T n_layers n_values eb fb u n_elems ct", "T", widths=(128,), prep=("enc", "n_elems")),
    EP("sparsify_tensors_dev", "n layers:T n_layers k:U64 residual loc vals packed pbits", "T"),
    EP("quantize_encrypt_cohort_dev", "iter first_idx n_clients n n_jobs layers:T n_layers src:P sdt:I32 eb u cts:P sum dmask", "S", widths=(128,),
       ok=ENOTSUP, cohort=True),
    EP("quantize_encrypt_cohort_u32_dev", "iter first_idx n_clients n n_jobs layers:T n_layers src:P sdt:I32 eb u cts:P sum", "S", widths=(20,),
       ok=ENOTSUP, cohort=True),
    EP("quantize_encrypt_cohort_u64_dev", "iter first_idx n_clients n n_jobs layers:T n_layers src:P sdt:I32 eb u cts:P sum", "S", widths=(40,),
       ok=ENOTSUP, cohort=True),
    EP("quantize_batch_encrypt_cohort_dev", "iter first_idx n_clients n_values n_elems n_jobs layers:T n_layers src:P sdt:I32 eb fb u cts:P sum dmask", "S",
       widths=(128,), ok=ENOTSUP, cohort=True),
    # the other forms of the same launch: the cipher indices as a list (cidx in place of first_idx), the cut chain (a trailing scratch; it
    # has no length rule, so n = 13 is admitted and the valid call runs)
    EP("quantize_encrypt_cohort_cut_dev", "iter first_idx n_clients n n_jobs layers:T n_layers src:P sdt:I32 eb u cts:P sum dmask scratch", "S",
       widths=(128,), cohort=True),
    EP("quantize_encrypt_cohort_cut_u32_dev", "iter first_idx n_clients n n_jobs layers:T n_layers src:P sdt:I32 eb u cts:P sum scratch", "S",
       widths=(20,), cohort=True),
    EP("quantize_encrypt_cohort_runs_dev", "iter cidx:U32 n_clients n n_jobs layers:T n_layers src:P sdt:I32 eb u cts:P sum dmask", "S", widths=(128,),
       ok=ENOTSUP, cohort=True),
    EP("quantize_encrypt_cohort_runs_u32_dev", "iter cidx:U32 n_clients n n_jobs layers:T n_layers src:P sdt:I32 eb u cts:P sum", "S", widths=(20,),
       ok=ENOTSUP, cohort=True),
    EP("quantize_batch_encrypt_cohort_runs_dev", "iter cidx:U32 n_clients n_values n_elems n_jobs layers:T n_layers src:P sdt:I32 eb fb u cts:P sum dmask",
       "S", widths=(128,), ok=ENOTSUP, cohort=True),
    EP("quantize_encrypt_cohort_cut_runs_dev", "iter cidx:U32 n_clients n n_jobs layers:T n_layers src:P sdt:I32 eb u cts:P sum dmask scratch", "S",
       widths=(128,), cohort=True),
    EP("quantize_encrypt_cohort_cut_runs_u32_dev", "iter cidx:U32 n_clients n n_jobs layers:T n_layers src:P sdt:I32 eb u cts:P sum scratch", "S",
       widths=(20,), cohort=True),
    EP("quantize_batch_encrypt_cohort_cut_runs_dev",
       "iter cidx:U32 n_clients n_values n_elems n_jobs layers:T n_layers src:P sdt:I32 eb fb u cts:P sum dmask scratch", "S", widths=(128,), cohort=True),
    EP("sparsify_cohort_tensors_dev", "n_clients n layers:T n_layers k:U64 src:P sdt:I32 residual rstride loc lstride vals vstride packed pstride pbits",
       "S", cohort=True),
    EP("quantize_cohort_dev", "n_clients n layers:T n_layers src:P sdt:I32 eb u u_stride zzz:D zf64 cts:P tails:P zeros", "S", cohort=True),
    # (at int_bits 20 the sparse chained launch admits every n >= 1; what it never takes is int_bits > 32)
    EP("quantize_encrypt_sparse_cohort_dev", "iter n_clients cidx:U32 n n_jobs layers:T n_layers src:P sdt:I32 eb u u_stride zzz:D zf64 cts:P zeros", "S",
       widths=(128,), ok=ENOTSUP, cohort=True),
    EP("quantize_encrypt_sparse_cohort_dev", "iter n_clients cidx:U32 n n_jobs layers:T n_layers src:P sdt:I32 eb u u_stride zzz:D zf64 cts:P zeros", "S",
       widths=(20,), cohort=True),
]
# the prepared cohort's online launch, all eight forms: the draws from a buffer, or generated inside the launch from a segment table
PREP = "n_clients n layers:T n_layers src:P sdt:I32 eb u masks:P cts:P sum"
PREP_BATCH = "n_clients n_values n_elems layers:T n_layers src:P sdt:I32 eb fb u masks:P cts:P sum"
EPS += [
    EP("quantize_combine_cohort_dev", PREP, "S", cohort=True),
    EP("quantize_combine_cohort_u32_dev", PREP, "S", widths=(20,), cohort=True),
    EP("quantize_batch_combine_cohort_dev", PREP_BATCH, "S", widths=(128,), cohort=True),
    EP("quantize_combine_cohort_philox_dev", PREP.replace(" u ", " segs:PX n_segs "), "S", cohort=True),
    EP("quantize_combine_cohort_philox_u32_dev", PREP.replace(" u ", " segs:PX n_segs "), "S", widths=(20,), cohort=True),
    EP("quantize_batch_combine_cohort_philox_dev", PREP_BATCH.replace(" u ", " segs:PX n_segs "), "S", widths=(128,), cohort=True),
    EP("quantize_combine_cohort_pcg64_dev", PREP.replace(" u ", " segs:PG n_segs "), "S", cohort=True),
    EP("quantize_combine_cohort_pcg64_u32_dev", PREP.replace(" u ", " segs:PG n_segs "), "S", widths=(20,), cohort=True),
]
BY_NAME = {ep.name: ep for ep in EPS}

CODEC_FRONT = {"quantize_encrypt_model_dev", "quantize_encrypt_prepared_model_dev", "quantize_encrypt_tensors_dev",
               "quantize_encrypt_prepared_tensors_dev"}
BATCH_FRONT = {"quantize_batch_model_dev", "quantize_batch_encrypt_prepared_model_dev", "quantize_batch_tensors_dev",
               "quantize_batch_encrypt_prepared_tensors_dev"}
DENSE = {"quantize_encrypt_cohort_dev", "quantize_encrypt_cohort_u32_dev", "quantize_encrypt_cohort_u64_dev", "quantize_batch_encrypt_cohort_dev",
         "quantize_encrypt_cohort_cut_dev", "quantize_encrypt_cohort_cut_u32_dev",
         "quantize_encrypt_cohort_runs_dev", "quantize_encrypt_cohort_runs_u32_dev", "quantize_batch_encrypt_cohort_runs_dev",
         "quantize_encrypt_cohort_cut_runs_dev", "quantize_encrypt_cohort_cut_runs_u32_dev", "quantize_batch_encrypt_cohort_cut_runs_dev"}
PREPARED = {"quantize_%scombine_cohort%s_dev" % f for f in (("", ""), ("", "_u32"), ("batch_", ""), ("", "_philox"), ("", "_philox_u32"), ("batch_", "_philox"),
                                                          ("", "_pcg64"), ("", "_pcg64_u32"))}
SPARSE_Q = {"quantize_cohort_dev", "quantize_encrypt_sparse_cohort_dev"}
NO_ALPHA = {"store_layers_dev", "sparsify_tensors_dev", "sparsify_cohort_tensors_dev"} | DENSE   # (the dense cohorts: cases_admitted)


def put(key, value):
    return lambda a, r: a.__setitem__(key, value)


def off(key, delta):
    return lambda a, r: a.__setitem__(key, a[key] + delta)


def item(key, i, value):
    return lambda a, r: a[key].__setitem__(i, value(a, r) if callable(value) else value)


def layer(l, field, value):
    return lambda a, r: a["layers"][l].__setitem__(field, value(a["layers"][l][field]) if callable(value) else value)


def cases(ep, bits):
    """(label, mutation, substring) of every refusal of `ep` at int_bits `bits`, and (label, mutation) of the accepted edge cases."""
    name, t, names = ep.name, ep.table, [n for n, _k in ep.args]
    wide = bits > 64
    bad, good = [], []
    who = {"sparsify_cohort_tensors_dev": "sparsify_cohort: ", "sparsify_tensors_dev": "sparsify_tensors: ", "quantize_cohort_dev": "quantize_cohort: ",
           "quantize_encrypt_sparse_cohort_dev": "quantize_cohort: "}.get(name, "")
    # -- the table --
    bad += [("n_layers 0", put("n_layers", 0), TABLE), ("null table", put("layers", None), TABLE)]
    if t != "B":
        bad += [("start0", layer(0, 0, 1), START0), ("descending", layer(2, 0, 4), ASCEND), ("past n", layer(2, 0, N + 1), ASCEND)]
    if t in "CB":
        bad += [("reserved", layer(0, 4, 1), "reserved field must be 0")]
    if name not in NO_ALPHA:
        bad += [("alpha 0", layer(0, 2, 0.0), "layer 0: " + ALPHA), ("alpha nan", layer(2, 2, math.nan), "layer 2: " + ALPHA)]
        good += [("alpha 0 on the empty layer", layer(1, 2, 0.0))]
    if name in ("quantize_encrypt_model_dev", "quantize_encrypt_prepared_model_dev"):
        bad += [("null x", layer(2, 1, None), "layer 2: null x_dev"), ("x + 2", layer(0, 1, lambda p: p + 2), "layer 0: x_dev is misaligned")]
    if name in ("quantize_batch_model_dev", "quantize_batch_encrypt_prepared_model_dev"):
        bad += [("null x", layer(2, 1, None), "layer 2: null or misaligned x_dev"), ("x + 2", layer(0, 1, lambda p: p + 2), "layer 0: null or misaligned x_dev")]
    if t == "T":
        bad += [("null ptr", layer(2, 1, None), "layer 2: null ptr"), ("ptr + 2", layer(2, 1, lambda p: p + 2), "layer 2: ptr is not aligned to its element size"),
                ("ptr + 1 (float16)", layer(0, 1, lambda p: p + 1), "layer 0: ptr is not aligned to its element size")]
    if t in "TS":
        bad += [("dtype 77", layer(1, 4, 77), "layer 1: unknown dtype 77"), ("flag 8", layer(2, 5, 8), "layer 2: unknown flags 0x8")]
    # -- widths and counts --
    if "eb" in names:
        msg = BITS_FRONT if name in CODEC_FRONT | DENSE | PREPARED | SPARSE_Q else BITS_BATCH if "fb" in names else BITS_BACK
        bad += [("element_bits 0", put("eb", 0), msg), ("element_bits 63", put("eb", 63), msg)]
        if not wide and msg == BITS_FRONT:
            bad += [("element_bits int_bits + 1", put("eb", bits + 1), msg)]
    if "fb" in names:
        bad += [("field_bits < element_bits", put("fb", EB - 1), BITS_BATCH), ("field_bits > int_bits", put("fb", bits + 1), BITS_BATCH)]
    if "n_elems" in names:
        for d in (1, -1):
            # (a prepared form compares n_elems with its cache first: the cache is prepared for the wrong count, so that the table disagrees alone)
            bad += [("n_elems %+d" % d, off("n_elems", d), COUNT)]
    if "count" in names:
        bad += [("first + count > n", put("first", 1), RANGE)]
    if "nc" in names:
        bad += [("num_clients 0", put("nc", 0), NCL)]
    if name == "decrypt_unquantize_model_dev":
        bad += [("no prefix", lambda a, r: a.update(n_add=0, n_minus=0), "at least one prefix")]
    # -- the prepared cache --
    if ep.prep:
        what = "encrypt" if ep.prep[0] == "enc" else "decrypt"
        bad += [("nothing prepared", put("_prep", None), "no prepared %s masks" % what),
                ("prepared for another length", lambda a, r: a.__setitem__("_prep", a[ep.prep[1]] + 2), "the prepared masks cover")]
    # -- vectors --
    vec = []
    if name in CODEC_FRONT:
        vec = [("u", None, NV), ("ct", None, NV), ("u", 4, U8), ("ct", "8w", A16), ("ct", "4n", A8)]
    elif name in BATCH_FRONT:
        vec = [("u", None, NV), ("ct", None, NV), ("u", 4, MV), ("ct", "8w", MV), ("ct", "4n", MV)]
    elif name == "decrypt_unquantize_model_dev":
        vec = [("vin", None, NV), ("fout", None, NV), ("vin", "8w", A16), ("vin", "4n", A8)]
    elif name in ("unquantize_model_dev", "unbatch_unquantize_model_dev"):
        vec = [("vin", None, NV), ("fout", None, NV), ("vin", "8w", MV), ("vin", "4n", MV), ("fout", 4, MV)]
    elif name in ("combine_unquantize_model_dev", "combine_unbatch_unquantize_model_dev"):
        vec = [("vin", None, NV), ("fout", None, NV), ("vin", "8w", MV), ("vadd", "8w", MV), ("vminus", "4n", MV), ("fout", 4, O8)]
    elif name in ("decrypt_prepared_unquantize_model_dev", "decrypt_prepared_unbatch_unquantize_model_dev"):
        vec = [("vin", None, NV), ("fout", None, NV), ("vin", "8w", A16), ("vin", "4n", A8), ("fout", 4, O8)]
    elif name == "store_layers_dev":
        vec = [("vin", None, "null or misaligned in_dev"), ("vin", 4, "null or misaligned in_dev"), ("stats", 4, "misaligned stats_dev")]
        bad += [("block 0", put("block", 0), "block must be in [1, 16384]")]
    elif name == "sparsify_tensors_dev":
        vec = [("k", None, who + "null k"), ("loc", None, NV), ("vals", None, NV)]
        bad += [("k > layer", item("k", 0, 6), who + "layer 0: k (6) > n (5)"), ("bits do not cover n", put("pbits", 3), who + "bits (3) must be in [1, 32]")]
    for key, how, msg in vec:
        if how is None:
            bad += [("null " + key, put(key, None), msg)]
        elif how == 4 or (how == "8w" and wide) or (how == "4n" and not wide):
            d = 8 if how == "8w" else 4
            bad += [("%s + %d" % (key, d), off(key, d), msg)]
    # -- cohorts --
    if name in DENSE:
        w = "flashe_" + name + ": "
        u32 = name.endswith("u32_dev")
        bad += [("n_clients 0", put("n_clients", 0), w + "n_clients must be >= 1"), ("null src", put("src", None), w + "null argument"),
                ("null cts", put("cts", None), w + "null argument"), ("null sum", put("sum", None), w + "null argument"),
                ("null u", put("u", None), w + "null argument"), ("u + 4", off("u", 4), U8),
                ("null ciphertext", item("cts", 1, None), "client 1: null ciphertext"),
                ("ciphertext aliases the sum", item("cts", 1, lambda a, r: a["sum"]), "client 1: the ciphertext aliases the sum")]
        if u32:
            bad += [("ct + 2", item("cts", 0, lambda a, r: a["cts"][0] + 2), "client 0: the ciphertext is not 4-byte aligned"),
                    ("sum + 2", off("sum", 2), "sum_out_dev must be 4-byte aligned"), ("n_jobs 0", put("n_jobs", 0), "n_jobs must be >= 1")]
        elif name.endswith("u64_dev"):
            # (the one-limb layout: uint64 vectors of a one-limb ctx, cohort_check_outs<uint64_t> without a mask)
            bad += [("ct + 4", item("cts", 0, lambda a, r: a["cts"][0] + 4), A8), ("sum + 4", off("sum", 4), "sum_out_dev must be aligned like a ciphertext vector"),
                    ("n_jobs 0", put("n_jobs", 0), "n_jobs must be >= 1")]
        else:
            bad += [("ct + 8", item("cts", 0, lambda a, r: a["cts"][0] + 8), A16), ("sum + 8", off("sum", 8), "sum_out_dev must be aligned like a ciphertext vector"),
                    ("dmask + 8", off("dmask", 8), "dmask_dev must be 16-byte aligned and apart from the sum"),
                    ("ciphertext aliases the mask", item("cts", 0, lambda a, r: a["dmask"]), "client 0: the ciphertext aliases the sum or the mask")]
        if "cidx" in names:
            ascending = w + "the cipher indices must be strictly ascending and below 2^32 - 1"
            bad += [("null idx", put("cidx", None), w + "null argument"), ("idx 1, 1", put("cidx", [1, 1]), ascending),
                    ("idx 1, 0", put("cidx", [1, 0]), ascending), ("idx 0, 2^32 - 1", put("cidx", [0, 2 ** 32 - 1]), ascending)]
        else:
            bad += [("first_idx 2^32 - 1", put("first_idx", 2 ** 32 - 1), "the cohort's cipher indices wrap around 2^32")]
        if "scratch" in names:
            # (two consecutive clients are one piece, which needs no scratch: a null one passes; the cut edge tests refuse it from two pieces upward)
            bad += [("scratch + 8", off("scratch", 8), "scratch_dev must be 16-byte aligned"),
                    ("scratch aliases the sum", lambda a, r: a.__setitem__("scratch", a["sum"]), "scratch_dev aliases the sum or the mask"),
                    ("scratch aliases a ciphertext", lambda a, r: a.__setitem__("scratch", a["cts"][1]), "scratch_dev aliases client 1's ciphertext")]
            if not u32:
                bad += [("scratch aliases the mask", lambda a, r: a.__setitem__("scratch", a["dmask"]), "scratch_dev aliases the sum or the mask")]
            good += [("null scratch at one piece", put("scratch", None))]
    if name in PREPARED:
        w = "flashe_" + name + ": "
        es = 4 if name.endswith("u32_dev") else 16 if wide else 8       # what masks, ciphertexts and sum are made of
        bad += [("n_clients 0", put("n_clients", 0), w + "n_clients must be >= 1"), ("null masks", put("masks", None), w + "null argument"),
                ("null ciphertext", item("cts", 1, None), "client 1: null mask or ciphertext"),
                ("mask + %d" % (es // 2), item("masks", 0, lambda a, r: a["masks"][0] + es // 2), "client 0: the mask or the ciphertext is not %d-byte aligned" % es),
                ("sum + %d" % (es // 2), off("sum", es // 2), "sum_out_dev must be %d-byte aligned" % es),
                ("sum aliases a ciphertext", lambda a, r: a.__setitem__("sum", a["cts"][1]), "client 1: the sum aliases the mask or the ciphertext"),
                ("sum aliases a source", lambda a, r: a.__setitem__("sum", a["src"][3]), "the sum aliases a source (client 1 layer 0)")]
        if "u" in names:
            bad += [("u + 4", off("u", 4), U8)]
        if "segs" in names:
            # one segment over the 2 n values cut in two: with a gap, and through client 0's last value
            def cut(first, gap=0, **second):
                return lambda a, r: a.update(n_segs=2, segs=[dict(a["segs"][0], n=first), dict(a["segs"][0], n=2 * N - first - gap, offset=first + gap, **second)])
            bad += [("n_segments -1", put("n_segs", -1), w + "-1 segments, a launch holds 0 .. 128"),
                    ("a gap", cut(N, gap=1), w + "the segments must tile the draws [0, n_clients x n) exactly"),
                    ("a split client", cut(N - 1), w + "a client's n draws must come from one segment")]
            if "philox" in name:
                bad += [("buffer_pos 5", lambda a, r: a["segs"][0].__setitem__("buffer_pos", 5), w + "a buffer_pos above 4")]
            else:
                bad += [("variant 2", lambda a, r: a["segs"][0].__setitem__("variant", 2), w + "a variant that is neither PCG64 (0) nor PCG64DXSM (1)"),
                        ("both variants", cut(N, variant=1), w + "PCG64 and PCG64DXSM segments in one table: a launch has one variant")]
    if name == "sparsify_cohort_tensors_dev":
        bad += [("n_clients 0", put("n_clients", 0), who + "n_clients must be in [1, 65535]"), ("null k", put("k", None), who + "null argument"),
                ("null src", put("src", None), who + "null argument"), ("null dtypes", put("sdt", None), who + "null argument"),
                ("row not a compute type", layer(0, 4, F16), "layer 0: the shared row names the COMPUTE type"),
                ("k > layer", item("k", 2, 9), who + "layer 2: k (9) > n (8)"), ("null loc", put("loc", None), NV), ("null vals", put("vals", None), NV),
                ("short loc_stride", put("lstride", 4), who + "a stride is shorter"), ("short vals_stride", put("vstride", 16), who + "a stride is shorter"),
                ("short residual_stride", put("rstride", 48), who + "a stride is shorter"), ("bits do not cover n", put("pbits", 3), who + "bits (3) must be in [1, 32]"),
                ("short packed_stride", put("pstride", 0), who + "packed_stride is shorter")]
    if name in SPARSE_Q:
        out = "upload" if name.endswith("sparse_cohort_dev") else "plaintext vector"
        bad += [("n_clients 0", put("n_clients", 0), who + "n_clients must be in [1, 65535]"), ("null src", put("src", None), who + "null argument"),
                ("null dtypes", put("sdt", None), who + "null argument"), ("null u", put("u", None), who + "null argument"),
                ("null zzz", put("zzz", None), who + "null argument"), ("null outputs", put("cts", None), who + "null argument"),
                ("null zeros", put("zeros", None), who + "null argument"), ("u + 4", off("u", 4), MV), ("zeros + 4", off("zeros", 4), MV),
                ("short u_stride", put("u_stride", N), who + "u_stride must cover a client's n + 1 draws"),
                ("row not a compute type", layer(2, 4, F16), "layer 2: the shared row names the COMPUTE type"),
                ("null output", item("cts", 1, None), "client 1: null or misaligned " + out),
                ("output + 4", item("cts", 0, lambda a, r: a["cts"][0] + 4), "client 0: null or misaligned " + out)]
        if name.endswith("sparse_cohort_dev"):
            bad += [("null idx", put("cidx", None), "flashe_" + name + ": null argument"), ("n_jobs 0", put("n_jobs", 0), "n_jobs must be >= 1"),
                    ("upload aliases zeros", item("cts", 1, lambda a, r: a["zeros"]), "client 1: the upload aliases zeros_dev")]
        else:
            bad += [("tail + 4", item("tails", 1, lambda a, r: a["tails"][1] + 4), "client 1: misaligned tail")]
    if name in SPARSE_Q or name == "sparsify_cohort_tensors_dev":
        # (client 1's layer 2 is entry 1 * 3 + 2 of the C x L arrays)
        bad += [("source dtype 77", item("sdt", 5, 77), "client 1 layer 2: unknown dtype 77"),
                ("float64 source under a float32 row", item("sdt", 5, F64), "client 1 layer 2: the source is of another compute class than the shared row"),
                ("null source", item("src", 5, None), "client 1 layer 2: null or misaligned source"),
                ("source + 2", item("src", 3, lambda a, r: a["src"][3] + 2), "client 1 layer 0: null or misaligned source")]
    return bad, good


@pytest.fixture(scope="module")
def rigs():
    made = {}

    def get(bits):
        if bits not in made:
            made[bits] = Rig(bits)
        return made[bits]
    yield get
    for r in made.values():
        r.eng.close()


def run_cases(r, ep):
    """Every case of `ep` on rig `r`; returns the list of what went wrong."""
    wrong = []
    bad, good = cases(ep, r.bits)
    for label, mutate, want in bad:
        a = r.defaults(ep)
        mutate(a, r)
        rc, msg = r.run(ep, a)
        dirty = r.dirty()
        if rc != EINVAL or want not in msg or dirty:
            wrong.append("%s [%s]: code %d, message %r (want %r), written: %s" % (ep.name, label, rc, msg, want, dirty))
        if a.get("segs") is not None and bytes(r.kept["segs"]) != bytes(_marshal(dict(ep.args)["segs"], a["segs"])):
            wrong.append("%s [%s]: the refused call changed the caller's segment table" % (ep.name, label))
        if ep.prep and label == "prepared for another length":
            held, n, _a, _m = r.eng.prepared_query(1 if ep.prep[0] == "enc" else 2)
            if not held or n != a["_prep"]:
                wrong.append("%s [%s]: the refused call did not leave the cache in place" % (ep.name, label))
        if dirty:
            r.poison()
    for label, mutate in good:
        a = r.defaults(ep)
        mutate(a, r)
        rc, msg = r.run(ep, a)
        if rc != ep.ok:
            wrong.append("%s [%s]: code %d, message %r (want code %d)" % (ep.name, label, rc, msg, ep.ok))
        if ep.ok == OK:
            r.poison()
        elif r.dirty():
            wrong.append("%s [%s]: declined, yet something was written" % (ep.name, label))
    return wrong


EP_AT = [(ep, bits) for ep in EPS for bits in ep.widths]


@pytest.mark.parametrize("ep,bits", EP_AT, ids=["%s-%d" % (ep.name, bits) for ep, bits in EP_AT])
def test_one_fault_is_einval_with_its_message_and_writes_nothing(rigs, ep, bits):
    r = rigs(bits)
    rc, msg = r.run(ep, r.defaults(ep))
    assert rc == ep.ok, (rc, msg)                                       # the call the cases start from is valid
    r.poison()
    wrong = run_cases(r, ep)
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("ep", [ep for ep in EPS if ep.ok == ENOTSUP or (ep.name in PREPARED and ep.name.endswith("u32_dev"))], ids=lambda ep: ep.name)
def test_refusal_comes_before_admission(rigs, ep, monkeypatch):
    """A valid call the chained launch does not take is FLASHE_ENOTSUP; the same call with one bad argument is FLASHE_EINVAL.  The prepared
    cohort's _u32 forms decline only a ctx without the compact layout: one created with the chained kernels switched off."""
    own = ep.name in PREPARED
    if own:
        monkeypatch.setenv("FLASHE_CHAIN", "0")
    r = Rig(ep.widths[0]) if own else rigs(ep.widths[0])
    try:
        assert not (own and r.eng.compact_supported())
        rc, msg = r.run(ep, r.defaults(ep))
        assert rc == ENOTSUP and "not a shape of the chained" in msg, (rc, msg)
        a = r.defaults(ep)
        a["eb"] = 63
        rc, msg = r.run(ep, a)
        assert rc == EINVAL and BITS_FRONT in msg, (rc, msg)
        assert not r.dirty()
    finally:
        if own:
            r.eng.close()


@pytest.mark.parametrize("bits", [128, 20])
def test_refusals_leave_the_ctx_as_it_was(rigs, bits):
    """One valid call per non-cohort entry point and of one prepared cohort form that draws inside its launch, every refusal, the valid calls
    again: bit-identical outputs (no half-written scratch or table)."""
    r = rigs(bits)
    eps = [ep for ep in EPS if (not ep.cohort or ep.name == "quantize_combine_cohort_philox_dev") and bits in ep.widths]

    def valid():
        got = {}
        for ep in eps:
            r.poison()
            rc, msg = r.run(ep, r.defaults(ep))
            assert rc == OK, (ep.name, rc, msg)
            got[ep.name] = r.snapshot()
        r.poison()
        return got

    before = valid()
    for ep in eps:
        assert any((v != POISON).any() for v in before[ep.name].values()), ep.name + " wrote nothing"
    wrong = [w for ep in eps for w in run_cases(r, ep)]
    assert not wrong, "\n".join(wrong)
    after = valid()
    for ep in eps:
        for k in before[ep.name]:
            assert np.array_equal(before[ep.name][k], after[ep.name][k]), (ep.name, k)


def admitted_n(ep, bits, cus=1):
    """The smallest n the chained launch of the dense cohort `ep` takes with one job on `cus` compute units (kernels.hip:
    cohort_chain_admits, small_cohort_admits, limb_cohort_admits: two whole tiles, or 2 x 128 AES blocks of 128 // int_bits values, for each of
    the 16 waves of a workgroup)."""
    if "_cut_" in ep.name:
        return N                             # (the cut chain has no length rule)
    if ep.name.endswith(("u32_dev", "u64_dev")):
        return (2 * 128 * cus * 16 - 1) * (128 // bits) + 1
    return ((2 * cus * 16 - 1) * 256 + 1) * (bits // FB if "batch" in ep.name else 1)


@pytest.mark.parametrize("ep", [BY_NAME[n] for n in sorted(DENSE)], ids=lambda ep: ep.name)
def test_dense_cohort_sources_and_alphas_at_an_admitted_shape(ep):
    """What the dense cohorts check behind the admission (cohort_rows, cohort_stage)."""
    bits = ep.widths[0]
    r = Rig(bits, n=admitted_n(ep, bits))
    r.eng.set_cu_limit(1)                    # (the launch fills one compute unit: the admitted shape stays small)
    try:
        rc, msg = r.run(ep, r.defaults(ep))
        assert rc == OK, (rc, msg)           # admitted, and run
        r.poison()
        bad = [("alpha 0", layer(0, 2, 0.0), "layer 0: " + ALPHA), ("alpha nan", layer(2, 2, math.nan), "layer 2: " + ALPHA),
               ("row not a compute type", layer(2, 4, F16), "layer 2: the shared row names the COMPUTE type"),
               ("source dtype 77", item("sdt", 5, 77), "client 1 layer 2: unknown dtype 77"),
               # (cohort_stage looks at the pointer first: the float64 source is aligned to its 8 bytes, so that its class is the one fault)
               ("float64 source under a float32 row", lambda a, r: (a["sdt"].__setitem__(5, F64), a["src"].__setitem__(5, r.x[1])),
                "client 1 layer 2: a float64 source under a float32 row"),
               ("null source", item("src", 5, None), "client 1 layer 2: null or misaligned source"),
               ("source + 2", item("src", 3, lambda a, r: a["src"][3] + 2), "client 1 layer 0: null or misaligned source")]
        wrong = []
        for label, mutate, want in bad:
            a = r.defaults(ep)
            mutate(a, r)
            rc, msg = r.run(ep, a)
            dirty = r.dirty()
            if rc != EINVAL or want not in msg or dirty:
                wrong.append("%s [%s]: code %d, message %r (want %r), written: %s" % (ep.name, label, rc, msg, want, dirty))
        assert not wrong, "\n".join(wrong)
    finally:
        r.eng.close()


def test_through_engine(rigs):
    """The arguments Engine passes through, refused through Engine: FlasheError carries the code and the message."""
    r = rigs(128)
    e, x = r.eng, r.layer_ptrs(r.x[0], 4)
    C = [(s, p, 1.0, False) for s, p in zip(STARTS, x)]
    B = [(s, p, 1.0, False) for s, p in zip(SIZES, x)]
    T = [(s, p, 1.0, 0.0, F32, 0) for s, p in zip(STARTS, x)]
    S = [(s, None, 1.0, 0.0, F32, 0) for s in STARTS]
    srcs, dts = [r.layer_ptrs(r.x[c], 4) for c in range(2)], [[F32] * 3] * 2
    tries = [
        (lambda: e.quantize_encrypt_model_dev(3, 0, 1, N, 1, 0, N, C, 63, r.u, r.ct[0]), BITS_FRONT),
        (lambda: e.quantize_encrypt_model_dev(3, 0, 1, N, 1, 1, N, C, EB, r.u, r.ct[0]), RANGE),
        (lambda: e.quantize_encrypt_model_dev(3, 0, 1, N, 1, 0, N, [], EB, r.u, r.ct[0]), TABLE),
        (lambda: e.quantize_encrypt_model_dev(3, 0, 1, N, 1, 0, N, C, EB, r.u + 4, r.ct[0]), U8),
        (lambda: e.decrypt_unquantize_model_dev(3, [], [], N, 1, 0, N, r.vin, C, EB, 2, r.fout), "at least one prefix"),
        (lambda: e.unquantize_model_dev(N, 0, N, r.vin + 8, C, EB, 2, r.fout), MV),
        (lambda: e.quantize_batch_model_dev(B, EB, FB, r.u, r.n_elems + 1, r.ct[0]), COUNT),
        (lambda: e.quantize_batch_model_dev(B, EB, EB - 1, r.u, r.n_elems, r.ct[0]), BITS_BATCH),
        (lambda: e.quantize_encrypt_tensors_dev(3, 0, 1, N, 1, 0, N, T[:1] + [(5, x[1], 1.0, 0.0, 77, 0)] + T[2:], EB, r.u, r.ct[0]), "unknown dtype 77"),
        (lambda: e.store_layers_dev(r.vin, N, T, 0, r.stats), "block must be in"),
        (lambda: e.sparsify_tensors_dev(N, [(s, p, F32) for s, p in zip(STARTS, x)], [6, 0, 3], r.residual, r.loc, r.vals), "layer 0: k (6) > n (5)"),
        (lambda: e.quantize_encrypt_cohort_dev(3, 2 ** 32 - 1, N, 1, S, srcs, dts, EB, r.u, r.ct, r.sum, r.dmask), "wrap around 2^32"),
        (lambda: e.quantize_encrypt_cohort_dev(3, 0, N, 1, S, srcs, dts, EB, r.u, [r.ct[0], r.sum], r.sum, r.dmask), "aliases the sum"),
        (lambda: e.sparsify_cohort_tensors_dev(N, [(s, F32) for s in STARTS], [2, 0, 3], srcs, dts, r.residual, 64, r.loc, 4, r.vals, 24), "a stride is shorter"),
        (lambda: e.quantize_cohort_dev(N, S, srcs, dts, EB, r.u, N, [0.5, 0.25], True, r.pt, r.tail, r.zeros), "u_stride must cover"),
    ]
    for i, (call, want) in enumerate(tries):
        with pytest.raises(FlasheError) as err:
            call()
        assert err.value.code == EINVAL and want in str(err.value), (i, str(err.value))
        assert not r.dirty(), i
    assert e.quantize_encrypt_cohort_dev(3, 0, N, 1, S, srcs, dts, EB, r.u, r.ct, r.sum, r.dmask) is False     # valid, too small: declined
