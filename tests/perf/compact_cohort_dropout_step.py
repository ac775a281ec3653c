#!/usr/bin/env python3
"""The client step of a COMPACT cohort of ten co-located clients (int_bits 20, element_bits 16, uint32 ciphertexts) in a round in which
clients DROPPED OUT: one of ten (client 5) and three of ten (clients 2, 5 and 6: three runs of indices), models of 1e7 and of 25,557,032
float32 values held as torch tensors on the GPU.  Two forms, alternated inside one process after a warm-up, timed with device events on the
engine's stream:
  staged   the only form that took non-consecutive indices at these widths before (prefer = "staged-chain"): a quantise launch per
           present client into 8-byte plaintexts, a narrowing pass per client, then flashe_encrypt_batch_sum_u32_dev over the gapped
           indices;
  fused    "cohort-chain": one launch from the floats and draws to the present clients' uint32 ciphertexts and their sum
           (flashe_quantize_encrypt_cohort_runs_u32_dev, prf_small_cohort_runs_kernel<20>).
Two levels:
  step      FlasheCohort(compact=True).quantize_encrypt(present=...) as a whole (the draws of the present clients are generated inside it,
            alike in both forms);
  launches  the launches that differ, on draws that are already there, table uploads included.
ALTS alternations (at least nine) give a median per form; `spread` is (max - min) / median of a form's own alternations, and the fused
form `wins` a level when staged / fused - 1 exceeds the larger of the two spreads.  The two forms' ciphertexts and sums are compared
inside the run.  A shape the planner does not chain is reported as such and not timed.  LEG=fused / LEG=staged runs one form of
`launches` alone (for a kernel trace).  Prints one line per case and level and a final JSON line."""
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
C = 10
ALTS = max(9, int(os.environ.get("ALTS", "9")))
LEG = os.environ.get("LEG", "")
LENGTHS = [int(v) for v in os.environ.get("LENGTHS", "10000000,25557032").split(",")]
WIDTHS = [int(v) for v in os.environ.get("WIDTHS", "20").split(",")]
DROPS = [[int(c) for c in v.split("+")] for v in os.environ.get("DROPS", "5,2+5+6").split(",")]
KEY = bytes(range(32))
EB = 16


def layer_sizes(n, k=40):
    w = [(i % 7 + 1) ** 3 for i in range(k)]
    sizes = [n * x // (2 * sum(w)) for x in w]
    return sizes + [n - sum(sizes)]


def args(b):
    return {"quantize": {"int_bits": b, "batch": False, "element_bits": EB, "padding": True, "secure": True}, "precompute": {"enable": False}}


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
    s, c = row["staged"], row["fused"]
    row["staged_over_fused"] = s["median_ms"] / c["median_ms"]
    row["spread"] = max(s["spread"], c["spread"])
    row["fused_wins"] = bool(row["staged_over_fused"] - 1.0 > row["spread"])
    return row


def alternate(forms):
    for fn in forms.values():
        fn()                                                   # warm-up of every form
    ms = {f: [] for f in forms}
    for _a in range(ALTS):
        for f, fn in forms.items():
            ms[f].append(fn())
    return {f: stats(v) for f, v in ms.items()}


def step_level(b, models, present):
    cohorts = {}
    for form, prefer, path in (("staged", "staged-chain", "staged-chain"), ("fused", None, "cohort-chain")):
        co = FlasheCohort(args(b), first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, compact=True)
        co.set_iter_index(1)
        co.prefer = prefer
        cohorts[form] = (co, path)
    last = {}

    def run(form):
        co, path = cohorts[form]
        np.random.seed(11)
        ms, up = timed(co.cipher.engine, lambda: co.quantize_encrypt([W(dict(models[p])) for p in present], present=present))
        assert up.path == path and up.present == present, (form, up.path)
        last[form] = up
        return ms
    res = alternate({f: (lambda f=f: run(f)) for f in cohorts})
    for a, b_ in zip(last["staged"].ciphertexts + [last["staged"].partial_sum], last["fused"].ciphertexts + [last["fused"].partial_sum]):
        assert a.compact and b_.compact and np.array_equal(a.to_host(), b_.to_host()), "the fused upload differs from the staged one"
    return res


def launch_level(b, models, sizes, present):
    from flashe_amd.engine import Engine
    eng = Engine(KEY, b, device=0)
    P, n = len(present), sum(sizes)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    names = sorted(models[0])
    alphas = [0.2 + 0.01 * (i % 5) for i in range(len(sizes))]
    rows = [(starts[i], None, alphas[i], 0.0, _lib.TENSOR_F32, 0) for i in range(len(sizes))]
    srcs = [[models[p][k].data_ptr() for k in names] for p in present]
    dts = [[_lib.TENSOR_F32] * len(sizes) for _ in present]
    tables = [[(starts[i], srcs[c][i], alphas[i], 0.0, _lib.TENSOR_F32, 0) for i in range(len(sizes))] for c in range(P)]
    du = eng.alloc(8 * P * n)
    np.random.seed(3)
    for at in range(0, P * n, 1 << 26):
        eng.numpy_random_dev(min(1 << 26, P * n - at), out=du.ptr + 8 * at)
    out = {f: ([eng.alloc(4 * n) for _ in range(P)], eng.alloc(4 * n)) for f in ("staged", "fused")}
    pts, pts32 = [eng.alloc_vec(n, 1) for _ in range(P)], [eng.alloc(4 * n) for _ in range(P)]

    def fused():
        took = eng.quantize_encrypt_cohort_runs_u32_dev(1, present, n, cm.N_JOBS, rows, srcs, dts, EB, du, out["fused"][0], out["fused"][1])
        assert took, "the chained launch declined the shape"

    def staged():                                              # (FlasheCohort._launch_staged's compact form)
        for c in range(P):
            eng.quantize_batch_tensors_dev(tables[c], n, EB, b, du.ptr + 8 * c * n, n, pts[c])
        for c in range(P):
            eng.narrow_u32_dev(n, pts[c], pts32[c])
        eng.encrypt_batch_sum_u32_dev(1, present, 1, n, cm.N_JOBS, pts32, out["staged"][0], out["staged"][1])

    forms = {"staged": staged, "fused": fused}
    if LEG:
        forms = {LEG: forms[LEG]}
    res = alternate({f: (lambda fn=fn: timed(eng, fn)[0]) for f, fn in forms.items()})
    if not LEG:
        # the two forms computed the same bytes, and the library's decrypt of the sum with the telescoped lists gives the plaintexts' sum
        for c in range(P):
            assert np.array_equal(out["staged"][0][c].download(np.uint32, n), out["fused"][0][c].download(np.uint32, n)), \
                f"client {present[c]}: the fused ciphertext differs from the staged one"
        gsum = out["fused"][1].download(np.uint32, n)
        assert np.array_equal(out["staged"][1].download(np.uint32, n), gsum), "the fused sum differs from the staged one"
        from flashe_amd.engine import telescope
        add, minus = telescope(list(present))
        wide, dec = eng.upload(gsum.astype(np.uint64)), eng.alloc_vec(n, 1)
        eng.decrypt_dev(1, add, minus, n, cm.N_JOBS, wide, dec)
        total = np.zeros(n, dtype=np.uint64)
        for c in range(P):
            total += pts[c].download(np.uint64, n)
        assert np.array_equal(dec.download(np.uint64, n), total & np.uint64((1 << b) - 1)), "the decrypt of the sum differs from the plaintexts' sum"
    return res


def main():
    res = {"clients": C, "alternations": ALTS, "library_sha256_16": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16], "cases": []}
    print(f"{C} clients, compact, element_bits {EB}, n_jobs {cm.N_JOBS}; {ALTS} alternations per form, device events")
    for n in LENGTHS:
        sizes = layer_sizes(n)
        g = torch.Generator(device="cuda").manual_seed(0)
        models = [{f"l{i:03d}": torch.randn(s, generator=g, device="cuda") * 0.05 + 0.001 * c for i, s in enumerate(sizes)} for c in range(C)]
        torch.cuda.synchronize()
        for b in WIDTHS:
            for dropped in DROPS:
                present = [c for c in range(C) if c not in dropped]
                case = {"n": n, "int_bits": b, "compact": True, "dropped": dropped}
                plan = FlasheCohort(args(b), first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, compact=True).plan(
                    [W(dict(models[p])) for p in present], present=present)
                case["plan"], case["runs"] = plan.path, plan.runs
                tag = f"n {n:>9} int_bits {b} compact dropped {dropped}"
                if plan.path != "cohort-chain":
                    case["reason"] = plan.reason
                    print(f"{tag}: the planner keeps {plan.path} ({plan.reason}); nothing to compare", flush=True)
                    res["cases"].append(case)
                    continue
                levels = [("launches", lambda: launch_level(b, models, sizes, present))]
                if not LEG:
                    levels.append(("step", lambda: step_level(b, models, present)))
                for name, fn in levels:
                    row = fn()
                    if not LEG:
                        verdict(row)
                    case[name] = row
                    print(f"{tag} {name:<8}", " ".join(f"{f} {r['median_ms']:8.3f} ms [{r['min_ms']:.3f} - {r['max_ms']:.3f}]"
                                                      for f, r in row.items() if isinstance(r, dict)),
                          "" if LEG else f"staged/fused {row['staged_over_fused']:.3f} spread {100 * row['spread']:.1f} % fused_wins {row['fused_wins']}", flush=True)
                res["cases"].append(case)
                torch.cuda.empty_cache()
        del models
    print(json.dumps(res))


if __name__ == "__main__":
    main()
