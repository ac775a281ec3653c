#!/usr/bin/env python3
"""The whole client-side round of the SPARSE job for ten co-located clients on the 29.2 M-value, 57-layer model of sparse_job_tensors.py,
held as float32 or bfloat16 torch tensors on the GPU, at the shipped shape (b = 20, sparsity 0.1) and config 5's (b = 128, sparsity 0.01):
sparsify, the masking choice, quantise + encrypt, the aggregate of the uploads, decrypt + unquantise + unnormalise into out=.
Two forms, alternated inside ONE process after a warm-up round, wall time around synchronised sections:
  (a) clients   ten Sparsifier.sparsify + FlasheClient.quantize_encrypt tensor steps one after the other (each client's packed locations
                decoded to the host lists the clients are handed), aggregate_sparse_uploads, one decrypt_unquantize(out=): what a caller
                ran before FlasheSparseCohort, and the yardstick;
  (b) cohort    FlasheSparseCohort: sparsify -> dynamic_masking() -> quantize_encrypt -> decrypt_unquantize(out=), with its sections timed.
Every block of REPS alternations gives one median per form; BLOCKS blocks give the box's spread (min - max of those medians).  Parity of
(b) against (a) -- packed locations, uploads, aggregate, the new model -- is checked on the warm-up round of every shape.
LEG=a / LEG=b runs one form alone (for a kernel trace; no parity check).  Prints one line per shape and a final JSON line."""
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from flashe_amd import _lib, cipher as cm  # noqa: E402
from flashe_amd.block import FlasheClient, FlasheSparseCohort, aggregate_sparse_uploads, dynamic_masking_choice  # noqa: E402
from flashe_amd.weights import Sparsifier, from_big_int  # noqa: E402


class W:
    def __init__(self, layers):
        self.walking_order = sorted(layers, key=str)
        self._weights = dict(layers)


cm.N_JOBS = 16
C = int(os.environ.get("CLIENTS", "10"))
sizes = [9408] + [s for s in (4096, 16384, 36864, 65536, 147456, 262144, 589824, 1048576, 2359296) for _ in range(6)] + [2048000, 1000]
names = [f"l{i:03d}" for i in range(len(sizes))]
total = sum(sizes)
REPS = int(os.environ.get("REPS", "5"))
BLOCKS = int(os.environ.get("BLOCKS", "3"))
LEG = os.environ.get("LEG", "")
SHAPES = os.environ.get("SHAPES", "")            # e.g. "20:0.1:float32" to run one shape
KEY = bytes(range(32))


def args(b):
    return {"quantize": {"int_bits": b, "batch": False, "element_bits": 16, "padding": True, "secure": True}, "precompute": {"enable": False},
            "mask": "dynamic"}


def sync():
    torch.cuda.synchronize()


def round_clients(cls, sps, models, out, it, seed):
    """-> (encoded tuples, uploads, aggregate)"""
    encs, masks, compact = [], [], []
    for sp, m in zip(sps, models):
        w = dict(m)
        enc = sp.sparsify(w, names)
        encs.append(enc)
        masks.append(np.asarray(from_big_int(enc[0], enc[1], enc[2], as_object=False)).astype(np.int64).reshape(-1))
        compact.append(w)
    choice = dynamic_masking_choice(masks, total)
    np.random.seed(seed)
    ups = []
    for cl, w in zip(cls, compact):
        cl.set_iter_index(it)
        cl.dynamic_masking(choice, masks)
        ww = W(w)
        ww._weights["zzz"] = np.array([0.0])
        ww.walking_order = sorted(ww._weights, key=str)
        o = cl.quantize_encrypt(ww, device=True, normalize=True)
        ups.append(o._weights[o.walking_order[0]])
    agg = aggregate_sparse_uploads(cls[0].cipher.engine, ups, masks, total, device=True)
    cls[0].set_idx_list(list(range(C)))
    cls[0].shape_dict = dict(sps[0].shape_dict_used_for_sparsification)
    cls[0].decrypt_unquantize(W({names[0]: agg}), out=out, unnormalize=True)
    for cl in cls[1:]:
        cl.quantizer.past_layer_mean_list = list(cls[0].quantizer.past_layer_mean_list)
        cl.quantizer.past_layer_std_list = list(cls[0].quantizer.past_layer_std_list)
    return encs, ups, agg


def round_cohort(co, models, out, it, seed, sections=None):
    marks = [time.perf_counter()]

    def mark():
        if sections is not None:
            sync()
            marks.append(time.perf_counter())

    co.set_iter_index(it)
    enc = co.sparsify(models, names)
    mark()
    co.dynamic_masking()
    mark()
    np.random.seed(seed)
    up = co.quantize_encrypt(normalize=True)
    mark()
    co.decrypt_unquantize(out=out, unnormalize=True)
    mark()
    if sections is not None:
        for k, a, b in zip(("sparsify", "choice", "quantize_encrypt_aggregate", "decrypt_unquantize"), marks, marks[1:]):
            sections.setdefault(k, []).append(1e3 * (b - a))
    assert up.path == "sparse-cohort", up.path
    return enc.encoded, up.uploads, up.aggregate


def timed(fn):
    sync()
    t0 = time.perf_counter()
    r = fn()
    sync()
    return 1e3 * (time.perf_counter() - t0), r


def main():
    res = {"clients": C, "n": total, "reps": REPS, "blocks": BLOCKS, "library_sha256_16": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]}
    print(f"model: {len(sizes)} layers, {total / 1e6:.1f} M values, {C} clients; element_bits = 16; {BLOCKS} blocks of {REPS} alternations")
    shapes = [(20, 0.1, "float32"), (20, 0.1, "bfloat16"), (128, 0.01, "float32"), (128, 0.01, "bfloat16")]
    if SHAPES:
        shapes = [(int(s.split(":")[0]), float(s.split(":")[1]), s.split(":")[2]) for s in SHAPES.split(",")]
    for b, sparsity, tname in shapes:
        dt = getattr(torch, tname)
        g = torch.Generator(device="cuda").manual_seed(0)
        models = [{nm: (torch.randn(s, generator=g, device="cuda") * 0.05 + 0.001 * c).to(dt) for nm, s in zip(names, sizes)} for c in range(C)]
        out_a = {k: torch.empty_like(t) for k, t in models[0].items()}
        out_b = {k: torch.empty_like(t) for k, t in models[0].items()}
        cls, sps = [], []
        for c in range(C):
            cl = FlasheClient(args(b))
            cl.create_cipher(c, C, KEY)
            cl.cipher.total = total
            cls.append(cl)
            sps.append(Sparsifier(sparsity))
        co = FlasheSparseCohort(args(b), first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, sparsity=sparsity)
        it = [0]
        sections = {}

        def form_a():
            return round_clients(cls, sps, models, out_a, it[0], 100 + it[0])

        def form_b():
            return round_cohort(co, models, out_b, it[0], 100 + it[0], sections if it[0] else None)

        forms = {"a": form_a, "b": form_b}
        if LEG:
            forms = {LEG: forms[LEG]}
        got = {f: fn() for f, fn in forms.items()}              # warm-up round; with both forms: parity
        sync()
        if len(got) == 2:
            (ea, ua, ga), (eb, ub, gb) = got["a"], got["b"]
            assert ea == eb, "packed locations differ"
            assert all(x.to_host().tobytes() == y.to_host().tobytes() for x, y in zip(ua, ub)), "uploads differ"
            assert ga.to_host().tobytes() == gb.to_host().tobytes(), "aggregates differ"
            assert all(torch.equal(out_a[k].view(torch.uint8), out_b[k].view(torch.uint8)) for k in out_a), "new models differ"
            parity = True
        else:
            parity = None
        del got
        medians = {f: [] for f in forms}
        for _b in range(BLOCKS):
            ms = {f: [] for f in forms}
            for _r in range(REPS):
                it[0] += 1
                for f, fn in forms.items():
                    ms[f].append(timed(fn)[0])
            for f in forms:
                medians[f].append(float(np.median(ms[f])))
        row = {f: {"median_ms": float(np.median(v)), "min_ms": min(v), "max_ms": max(v)} for f, v in medians.items()}
        row["sections_b_ms"] = {k: float(np.median(v)) for k, v in sections.items()}
        row["parity"] = parity
        res[f"b{b}_s{sparsity}_{tname}"] = row
        print(f"b = {b:3d}, sparsity {sparsity}, {tname:8s}:",
              " ".join(f"({f}) {r['median_ms']:8.2f} ms [{r['min_ms']:.2f} - {r['max_ms']:.2f}]" for f, r in row.items() if f in forms),
              "| (b) sections:", " ".join(f"{k} {v:.2f}" for k, v in row["sections_b_ms"].items()), f"| parity {parity}")
        del models, out_a, out_b, cls, sps, co, forms
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
