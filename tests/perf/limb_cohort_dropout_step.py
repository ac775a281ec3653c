#!/usr/bin/env python3
"""The client step of a ONE-LIMB cohort of ten co-located clients (int_bits 36: three values per AES block, and 64: two; element_bits =
int_bits - 4; uint64 ciphertexts) in a round in which clients DROPPED OUT: one of ten (client 5) and three of ten (clients 2, 5 and 6:
three runs of indices), models of 1e7 and of 25,557,032 float32 values held as torch tensors on the GPU.  Two forms, alternated inside one
process after a warm-up, timed with device events on the engine's stream:
  staged   the only form that took non-consecutive indices at these widths before (prefer = "staged-chain"): a quantise launch per
           present client into 8-byte plaintexts, then flashe_encrypt_batch_sum_dev over the gapped indices (36 bytes moved per value and
           client);
  chain    "cohort-chain": one launch from the floats and draws to the present clients' uint64 ciphertexts and their sum
           (flashe_quantize_encrypt_cohort_runs_u64_dev, prf_limb_cohort_runs_kernel<3 | 2>; 20 bytes).
Two levels:
  step      FlasheCohort(one_limb=True).quantize_encrypt(present=...) as a whole (the draws of the present clients are generated inside
            it, alike in both forms);
  launches  the launches that differ, on draws that are already there, table uploads included.
ALTS alternations (at least seven) give a median per form; `spread` is (max - min) / median of a form's own alternations, and the chain
`wins` a level when staged / chain - 1 exceeds the larger of the two spreads.  `share` is the part of a form's whole step that its
differing launches account for (launches median / step median).  The two forms' ciphertexts and sums are compared inside the run.  A
shape the planner does not chain is reported as such and not timed.  LEG=chain / LEG=staged runs one form of `launches` alone (for a
kernel trace).  Prints one line per case and level and a final JSON line."""
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
ALTS = max(7, int(os.environ.get("ALTS", "7")))
LEG = os.environ.get("LEG", "")
LENGTHS = [int(v) for v in os.environ.get("LENGTHS", "10000000,25557032").split(",")]
WIDTHS = [int(v) for v in os.environ.get("WIDTHS", "36,64").split(",")]
DROPS = [[int(c) for c in v.split("+")] for v in os.environ.get("DROPS", "5,2+5+6").split(",")]
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


def cohort(b):
    return FlasheCohort(args(b), first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, one_limb=True)


def step_level(b, models, present):
    cohorts = {}
    for form, prefer, path in (("staged", "staged-chain", "staged-chain"), ("chain", None, "cohort-chain")):
        co = cohort(b)
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
    for a, b_ in zip(last["staged"].ciphertexts + [last["staged"].partial_sum], last["chain"].ciphertexts + [last["chain"].partial_sum]):
        assert a.elem_bytes == 8 and b_.elem_bytes == 8 and np.array_equal(a.to_host(), b_.to_host()), "the chained upload differs from the staged one"
    return res


def launch_level(b, models, sizes, present):
    from flashe_amd.engine import Engine
    eng = Engine(KEY, b, device=0)
    P, n, EB = len(present), sum(sizes), element_bits(b)
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
    out = {f: ([eng.alloc_vec(n) for _ in range(P)], eng.alloc_vec(n)) for f in ("staged", "chain")}
    pts = [eng.alloc_vec(n) for _ in range(P)]

    def chain():
        took = eng.quantize_encrypt_cohort_runs_u64_dev(1, present, n, cm.N_JOBS, rows, srcs, dts, EB, du, out["chain"][0], out["chain"][1])
        assert took, "the chained launch declined the shape"

    def staged():                                              # (FlasheCohort._launch_staged's one-limb form)
        for c in range(P):
            eng.quantize_batch_tensors_dev(tables[c], n, EB, b, du.ptr + 8 * c * n, n, pts[c])
        eng.encrypt_batch_sum_dev(1, present, 1, n, cm.N_JOBS, pts, 1, out["staged"][0], out["staged"][1])

    forms = {"staged": staged, "chain": chain}
    if LEG:
        forms = {LEG: forms[LEG]}
    res = alternate({f: (lambda fn=fn: timed(eng, fn)[0]) for f, fn in forms.items()})
    if not LEG:
        # the two forms computed the same values, and the library's decrypt of the sum with the telescoped lists gives the plaintexts' sum
        for c in range(P):
            assert np.array_equal(out["staged"][0][c].download(np.uint64, n).copy(), out["chain"][0][c].download(np.uint64, n)), \
                f"client {present[c]}: the chained ciphertext differs from the staged one"
        assert np.array_equal(out["staged"][1].download(np.uint64, n).copy(), out["chain"][1].download(np.uint64, n)), "the chained sum differs from the staged one"
        from flashe_amd.engine import telescope
        add, minus = telescope(list(present))
        dec = eng.alloc_vec(n)
        eng.decrypt_dev(1, add, minus, n, cm.N_JOBS, out["chain"][1], dec)
        total = np.zeros(n, dtype=np.uint64)
        for c in range(P):
            total += pts[c].download(np.uint64, n)
        if b < 64:
            total &= np.uint64((1 << b) - 1)
        assert np.array_equal(dec.download(np.uint64, n), total), "the decrypt of the sum differs from the plaintexts' sum"
    return res


def main():
    res = {"clients": C, "alternations": ALTS, "library_sha256_16": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16], "cases": []}
    print(f"{C} clients, one limb, element_bits int_bits - 4, n_jobs {cm.N_JOBS}; {ALTS} alternations per form, device events")
    for n in LENGTHS:
        sizes = layer_sizes(n)
        g = torch.Generator(device="cuda").manual_seed(0)
        models = [{f"l{i:03d}": torch.randn(s, generator=g, device="cuda") * 0.05 + 0.001 * c for i, s in enumerate(sizes)} for c in range(C)]
        torch.cuda.synchronize()
        for b in WIDTHS:
            for dropped in DROPS:
                present = [c for c in range(C) if c not in dropped]
                case = {"n": n, "int_bits": b, "m": 128 // b, "dropped": dropped}
                plan = cohort(b).plan([W(dict(models[p])) for p in present], present=present)
                case["plan"], case["runs"] = plan.path, plan.runs
                tag = f"n {n:>9} int_bits {b} dropped {dropped}"
                if plan.path != "cohort-chain" and not LEG:
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
                          "" if LEG else f"staged/chain {row['staged_over_chain']:.3f} spread {100 * row['spread']:.1f} % chain_wins {row['chain_wins']}", flush=True)
                if not LEG:
                    case["share"] = {f: case["launches"][f]["median_ms"] / case["step"][f]["median_ms"] for f in ("staged", "chain")}
                    print(f"{tag} share of the whole step in the differing launches: staged {100 * case['share']['staged']:.1f} % chain {100 * case['share']['chain']:.1f} %",
                          flush=True)
                res["cases"].append(case)
                torch.cuda.empty_cache()
        del models
    print(json.dumps(res))


if __name__ == "__main__":
    main()
