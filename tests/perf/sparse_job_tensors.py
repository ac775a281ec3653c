#!/usr/bin/env python3
"""The SPARSE job's client step from a training framework's tensors: the ResNet-50 layer sizes of tests/perf/sparse_job_step.py (29.2 M
values, 57 layers) as float32 or bfloat16 torch tensors, 10 clients, at the shipped shape (b = 20, sparsity 0.1) and config 5's (b = 128,
sparsity 0.01).  Per phase, two ways on one box:
  host path   the caller copies every layer to the host (t.float().cpu().numpy()), Sparsifier.sparsify, quantize_encrypt of the compact
              layers + 'zzz', decrypt_unquantize(unnormalize=True) to float64 host arrays, the caller copies them back into its parameters;
  tensors     Sparsifier.sparsify reads the tensors in place (flashe_sparsify_tensors_dev), quantize_encrypt reads its compact layers in
              HBM, decrypt_unquantize(out=params, unnormalize=True) writes the parameters in place.
Then the sparsifier A/B: flashe_sparsify_tensors_dev against flashe_sparsify_batch_dev on the same float32 values in one flat buffer,
alternated in one process (device events); `--ab-only` runs only that part (the rocprofv3 kernel statistics).  The arbiter's pass (aggregate_sparse_uploads) is the same for both and not timed."""
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from flashe_amd import cipher as cm  # noqa: E402
from flashe_amd.block import FlasheClient, aggregate_sparse_uploads  # noqa: E402
from flashe_amd.engine import Engine  # noqa: E402
from flashe_amd.weights import Sparsifier, from_big_int  # noqa: E402


class W:
    def __init__(self, layers):
        self.walking_order = sorted(layers, key=str)
        self._weights = dict(layers)


cm.N_JOBS = 16
C = 10
REPS = int(os.environ.get("REPS", "3"))
sizes = [9408] + [s for s in (4096, 16384, 36864, 65536, 147456, 262144, 589824, 1048576, 2359296) for _ in range(6)] + [2048000, 1000]
names = [f"l{i:03d}" for i in range(len(sizes))]
total = sum(sizes)
KEY = bytes(range(32))


def args(b):
    return {"quantize": {"int_bits": b, "batch": False, "element_bits": 16, "padding": True, "secure": True}, "precompute": {"enable": False},
            "mask": "dynamic"}


def sync():
    torch.cuda.synchronize()


def run(b, sparsity, tdtype, path):
    """-> median ms of (sparsify, quantize_encrypt, decrypt_unquantize) per client step over REPS rounds after one warm-up round; the
    host path includes the caller's .cpu() copy in sparsify and the copy back in decrypt_unquantize."""
    g = torch.Generator(device="cuda").manual_seed(1)
    params = [{nm: (torch.randn(s, device="cuda", generator=g) * 0.05).to(tdtype) for nm, s in zip(names, sizes)} for _ in range(C)]
    cls, sps = [], []
    for c in range(C):
        cl = FlasheClient(args(b))
        cl.create_cipher(c, C, KEY)
        cl.cipher.total = total
        cls.append(cl)
        sps.append(Sparsifier(sparsity))
    arb = Engine(KEY, b)
    t_sp, t_enc, t_dec = [], [], []
    for rnd in range(REPS + 1):
        masks, compact = [], []
        sp_ms = 0.0
        for c in range(C):
            sync()
            t0 = time.perf_counter()
            w = dict(params[c]) if path == "tensors" else {k: p.float().cpu().numpy() for k, p in params[c].items()}
            enc = sps[c].sparsify(w, names)
            sync()
            sp_ms += time.perf_counter() - t0
            masks.append(np.asarray(from_big_int(enc[0], enc[1], enc[2], as_object=False)).astype(np.int64))
            compact.append(w)
        uploads, enc_ms = [], 0.0
        for c, cl in enumerate(cls):
            cl.set_iter_index(rnd + 1)
            cl.dynamic_masking("single", masks)
            w = W(compact[c])
            w._weights["zzz"] = np.array([0.0])
            w.walking_order = sorted(w._weights, key=str)
            np.random.seed(c)
            sync()
            t0 = time.perf_counter()
            out = cl.quantize_encrypt(w, device=True, normalize=True)
            cl.cipher.engine.sync()
            enc_ms += time.perf_counter() - t0
            uploads.append(out._weights[out.walking_order[0]])
        agg = aggregate_sparse_uploads(arb, uploads, masks, total, device=True)
        arb.sync()
        cl = cls[0]
        cl.set_idx_list(list(range(C)))
        cl.shape_dict = dict(sps[0].shape_dict_used_for_sparsification)
        sync()
        t0 = time.perf_counter()
        if path == "tensors":
            cl.decrypt_unquantize(W({names[0]: agg}), out=params[0], unnormalize=True)
        else:
            res = cl.decrypt_unquantize(W({names[0]: agg}), unnormalize=True)
            for k, p in params[0].items():
                p.copy_(torch.from_numpy(np.ascontiguousarray(res._weights[k])).to(p.dtype))
        sync()
        dec_ms = time.perf_counter() - t0
        if rnd:
            t_sp.append(1e3 * sp_ms / C)
            t_enc.append(1e3 * enc_ms / C)
            t_dec.append(1e3 * dec_ms)
    return float(np.median(t_sp)), float(np.median(t_enc)), float(np.median(t_dec))


def ab_sparsifier(sparsity, reps=20):
    """flashe_sparsify_tensors_dev (layers as separate tensors) against flashe_sparsify_batch_dev (the same float32 values in one flat
    buffer), alternated, device time per call (events around the launches; both upload their layer table first)."""
    eng = Engine(KEY, 128)
    g = torch.Generator(device="cuda").manual_seed(2)
    flat = torch.randn(total, device="cuda", generator=g) * 0.05
    views, at = [], 0
    for s in sizes:
        views.append(flat[at:at + s])
        at += s
    ks = [max(1, int(np.floor(sparsity * s))) for s in sizes]
    K = sum(ks)
    res_a, res_b = eng.alloc(4 * total), eng.alloc(4 * total)
    eng.memset_dev(res_a, 0, 4 * total)
    eng.memset_dev(res_b, 0, 4 * total)
    loc_a, loc_b, val_a, val_b = eng.alloc(4 * K), eng.alloc(4 * K), eng.alloc(4 * K), eng.alloc(4 * K)
    bits = total.bit_length()
    packed = eng.alloc(8 * ((K * bits + 63) // 64))
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    # both calls' ctypes arguments are built before the events: the window holds the C call (table upload + launches) only, not the
    # Python that fills a 57-entry ctypes table (~30 us with the GPU idle, which an earlier version of this script timed as kernel time)
    arr, nl = eng._tensor_layers([(st, v.data_ptr(), 1.0, 0.0, 0, 0) for st, v in zip(starts, views)])
    L = len(sizes)
    an, ak = (ctypes.c_uint64 * L)(*sizes), (ctypes.c_uint64 * L)(*ks)
    lib, h = eng._lib, eng._h
    torch.cuda.synchronize()
    ev = [eng.event() for _ in range(4)]
    ta, tb = [], []
    for r in range(reps + 2):
        eng.record(ev[0])
        eng._check(lib.flashe_sparsify_tensors_dev(h, total, arr, nl, ak, res_a.ptr, loc_a.ptr, val_a.ptr, packed.ptr, bits))
        eng.record(ev[1])
        eng.record(ev[2])
        eng._check(lib.flashe_sparsify_batch_dev(h, L, an, ak, flat.data_ptr(), 0, res_b.ptr, loc_b.ptr, val_b.ptr))
        eng.record(ev[3])
        eng.sync()
        if r >= 2:
            ta.append(eng.elapsed_ms(ev[0], ev[1]))
            tb.append(eng.elapsed_ms(ev[2], ev[3]))
    same = np.array_equal(val_a.download(np.float32, K), val_b.download(np.float32, K)) and \
        np.array_equal(res_a.download(np.float32, total), res_b.download(np.float32, total))
    return float(np.median(ta)), float(np.median(tb)), same


def ab_bf16(sparsity, reps=20):
    """the tensor sparsifier on the same model as bfloat16 tensors (half the bytes per pass)"""
    eng = Engine(KEY, 128)
    g = torch.Generator(device="cuda").manual_seed(3)
    ts = [(torch.randn(s, device="cuda", generator=g) * 0.05).to(torch.bfloat16) for s in sizes]
    ks = [max(1, int(np.floor(sparsity * s))) for s in sizes]
    K = sum(ks)
    res, loc, val = eng.alloc(4 * total), eng.alloc(4 * K), eng.alloc(4 * K)
    eng.memset_dev(res, 0, 4 * total)
    bits = total.bit_length()
    packed = eng.alloc(8 * ((K * bits + 63) // 64))
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    arr, nl = eng._tensor_layers([(st, t.data_ptr(), 1.0, 0.0, 3, 0) for st, t in zip(starts, ts)])
    ak = (ctypes.c_uint64 * len(sizes))(*ks)
    torch.cuda.synchronize()
    e0, e1 = eng.event(), eng.event()
    t = []
    for r in range(reps + 2):
        eng.record(e0)
        eng._check(eng._lib.flashe_sparsify_tensors_dev(eng._h, total, arr, nl, ak, res.ptr, loc.ptr, val.ptr, packed.ptr, bits))
        eng.record(e1)
        eng.sync()
        if r >= 2:
            t.append(eng.elapsed_ms(e0, e1))
    return float(np.median(t))


if __name__ == "__main__":
    print(f"model: {total} values in {len(sizes)} layers, {C} clients; medians of {REPS} rounds after a warm-up round")
    for sparsity in (0.1, 0.01):
        a, b_, same = ab_sparsifier(sparsity)
        print(f"sparsifier A/B, float32, sparsity {sparsity}: tensors {a:.3f} ms, flat batch {b_:.3f} ms ({100 * (a / b_ - 1):+.1f} %), "
              f"identical outputs: {same}")
        print(f"sparsifier, bfloat16 tensors, sparsity {sparsity}: {ab_bf16(sparsity):.3f} ms")
    if "--ab-only" in sys.argv:                     # (the kernel statistics run: the sparsifier launches only)
        sys.exit(0)
    for b, sparsity in ((20, 0.1), (128, 0.01)):
        for tname, tdtype in (("float32", torch.float32), ("bfloat16", torch.bfloat16)):
            h = run(b, sparsity, tdtype, "host")
            t = run(b, sparsity, tdtype, "tensors")
            print(f"b = {b:3d}, sparsity {sparsity}, {tname:8s}: sparsify {h[0]:7.2f} -> {t[0]:6.2f} ms | quantize_encrypt {h[1]:6.2f} -> "
                  f"{t[1]:6.2f} ms | decrypt_unquantize {h[2]:7.2f} -> {t[2]:6.2f} ms | step {sum(h):7.2f} -> {sum(t):6.2f} ms "
                  f"(host path -> tensors)")
