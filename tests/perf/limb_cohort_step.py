#!/usr/bin/env python3
"""The client step of a cohort of ten co-located clients at int_bits 33 .. 64 in the one-limb layout (int_bits 36 and 40: three values per
AES block; 48 and 64: two; element_bits = int_bits - 4, what ten clients leave; not batched), models of 1e7 and of 25,557,032 float32
values held as torch tensors on the GPU.  Two forms, alternated inside one process after a warm-up, timed with device events on the
engine's stream:
  staged   the parent's form of this cohort: FlasheCohort(one_limb=False) -> "staged-chain", a quantise launch per client into one-limb
           plaintexts, then the summed one-limb encrypt (36 bytes moved per value and client);
  chain    FlasheCohort(one_limb=True) -> "cohort-chain": one launch from the floats to the uint64 ciphertexts and their sum (20 bytes).
Two levels:
  step      FlasheCohort.quantize_encrypt as a whole (the draws of all clients are generated inside it, alike in both forms);
  launches  the launches that differ, on draws that are already there (Engine.quantize_encrypt_cohort_u64_dev against
            C x Engine.quantize_batch_tensors_dev + Engine.encrypt_batch_sum_dev), table uploads included.
ALTS alternations (at least seven) give a median per form; `spread` is (max - min) / median of a form's own alternations, and the chain
`wins` a level when staged / chain - 1 exceeds the larger of the two spreads.  LEG=chain / LEG=staged runs one form of `launches` alone
(for a kernel trace).  Prints one line per case and level and a final JSON line."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from flashe_amd import _lib, cipher as cm  # noqa: E402
from flashe_amd.block import FlasheCohort  # noqa: E402


class W:
    def __init__(self, layers):
        self.walking_order = sorted(layers)
        self._weights = dict(layers)


cm.N_JOBS = 16
C = int(os.environ.get("CLIENTS", "10"))
ALTS = max(7, int(os.environ.get("ALTS", "9")))
LEG = os.environ.get("LEG", "")
LENGTHS = [int(v) for v in os.environ.get("LENGTHS", "10000000,25557032").split(",")]
WIDTHS = [int(v) for v in os.environ.get("WIDTHS", "36,40,48,64").split(",")]
KEY = bytes(range(32))


def layer_sizes(n, k=40):
    w = [(i % 7 + 1) ** 3 for i in range(k)]
    sizes = [n * x // (2 * sum(w)) for x in w]
    return sizes + [n - sum(sizes)]


def element_bits(b):
    return b - 4                                              # (ten clients: their sum must still fit int_bits)


def args(b):
    return {"quantize": {"int_bits": b, "batch": False, "element_bits": element_bits(b), "padding": True, "secure": True}, "precompute": {"enable": False}}


def timed(eng, fn):
    e0, e1 = eng.event(), eng.event()
    torch.cuda.synchronize()
    eng.record(e0)
    r = fn()
    eng.record(e1)
    ms = eng.elapsed_ms(e0, e1)
    eng.event_destroy(e0)
    eng.event_destroy(e1)
    return ms, r


def stats(ms):
    med = float(np.median(ms))
    return {"median_ms": med, "min_ms": float(min(ms)), "max_ms": float(max(ms)), "spread": float((max(ms) - min(ms)) / med)}


def verdict(row):
    s, c = row["staged"], row["chain"]
    row["staged_over_chain"] = s["median_ms"] / c["median_ms"]
    row["spread"] = max(s["spread"], c["spread"])
    row["chain_wins"] = bool(row["staged_over_chain"] - 1.0 > row["spread"])
    return row


def alternate(forms):
    for fn in forms.values():
        fn()                                                   # warm-up of every form
    ms = {f: [] for f in forms}
    for _a in range(ALTS):
        for f, fn in forms.items():
            ms[f].append(fn())
    return {f: stats(v) for f, v in ms.items()}


def step_level(b, models):
    cohorts = {}
    for form, one_limb, path in (("staged", False, "staged-chain"), ("chain", True, "cohort-chain")):
        co = FlasheCohort(args(b), first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, one_limb=one_limb)
        co.set_iter_index(1)
        cohorts[form] = (co, path)

    def run(form):
        co, path = cohorts[form]
        ms, up = timed(co.cipher.engine, lambda: co.quantize_encrypt([W(dict(m)) for m in models]))
        assert up.path == path, (form, up.path)
        return ms
    return alternate({f: (lambda f=f: run(f)) for f in cohorts})


def launch_level(b, models, sizes):
    from flashe_amd.engine import Engine
    eng = Engine(KEY, b, device=0)
    n, EB = sum(sizes), element_bits(b)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    names = sorted(models[0])
    alphas = [0.2 + 0.01 * (i % 5) for i in range(len(sizes))]
    rows = [(starts[i], None, alphas[i], 0.0, _lib.TENSOR_F32, 0) for i in range(len(sizes))]
    srcs = [[m[k].data_ptr() for k in names] for m in models]
    dts = [[_lib.TENSOR_F32] * len(sizes) for _ in models]
    tables = [[(starts[i], srcs[c][i], alphas[i], 0.0, _lib.TENSOR_F32, 0) for i in range(len(sizes))] for c in range(C)]
    du = eng.alloc(8 * C * n)
    np.random.seed(3)
    for at in range(0, C * n, 1 << 26):
        eng.numpy_random_dev(min(1 << 26, C * n - at), out=du.ptr + 8 * at)
    idxs = list(range(C))
    ctsch, sumch = [eng.alloc_vec(n) for _ in range(C)], eng.alloc_vec(n)
    pts, cts64, sum64 = [eng.alloc_vec(n) for _ in range(C)], [eng.alloc_vec(n) for _ in range(C)], eng.alloc_vec(n)

    def chain():
        assert eng.quantize_encrypt_cohort_u64_dev(1, 0, n, cm.N_JOBS, rows, srcs, dts, EB, du, ctsch, sumch), "the chained launch declined the shape"

    def staged():
        for c in range(C):
            eng.quantize_batch_tensors_dev(tables[c], n, EB, b, du.ptr + 8 * c * n, n, pts[c])
        eng.encrypt_batch_sum_dev(1, idxs, 1, n, cm.N_JOBS, pts, 1, cts64, sum64)

    forms = {"staged": staged, "chain": chain}
    if LEG:
        forms = {LEG: forms[LEG]}
    res = alternate({f: (lambda fn=fn: timed(eng, fn)[0]) for f, fn in forms.items()})
    if not LEG:
        # the two forms computed the same values
        assert np.array_equal(sum64.download(np.uint64, n).copy(), sumch.download(np.uint64, n)), "the chained sum differs from the staged one"
        assert np.array_equal(cts64[C - 1].download(np.uint64, n).copy(), ctsch[C - 1].download(np.uint64, n)), "the last chained ciphertext differs"
    return res


def main():
    res = {"clients": C, "alternations": ALTS, "library_sha256_16": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16], "cases": []}
    print(f"{C} clients, element_bits int_bits - 4, n_jobs {cm.N_JOBS}; {ALTS} alternations per form, device events")
    for n in LENGTHS:
        sizes = layer_sizes(n)
        g = torch.Generator(device="cuda").manual_seed(0)
        models = [{f"l{i:03d}": torch.randn(s, generator=g, device="cuda") * 0.05 + 0.001 * c for i, s in enumerate(sizes)} for c in range(C)]
        torch.cuda.synchronize()
        for b in WIDTHS:
            case = {"n": n, "int_bits": b}
            levels = [("launches", lambda: launch_level(b, models, sizes))]
            if not LEG:
                levels.append(("step", lambda: step_level(b, models)))
            for name, fn in levels:
                row = fn()
                if not LEG:
                    verdict(row)
                case[name] = row
                print(f"n {n:>9} int_bits {b} {name:<8}", " ".join(f"{f} {r['median_ms']:8.3f} ms [{r['min_ms']:.3f} - {r['max_ms']:.3f}]"
                                                                     for f, r in row.items() if isinstance(r, dict)),
                      "" if LEG else f"staged/chain {row['staged_over_chain']:.3f} spread {100 * row['spread']:.1f} % chain_wins {row['chain_wins']}", flush=True)
            res["cases"].append(case)
            torch.cuda.empty_cache()
        del models
    print(json.dumps(res))


if __name__ == "__main__":
    main()
