#!/usr/bin/env python3
"""The client step of a SHORT cohort in which clients dropped out, and of a short BATCHED cohort, in two forms alternated inside ONE
process after a warm-up:
  cut      FlasheCohort(cut="any") -> "cut-chain": the summed chain cut at the gaps (and by the rule of csrc/cohort_cut.h) + one combine pass;
  staged   the same cohort with prefer="staged-chain": a quantise (+ batch) launch per present client into plaintexts, then the summed
           batch encrypt -- what cut=True and the parent commit run for exactly these shapes.
Two levels:
  launches  the launches that differ (FlasheCohort._launch_chain against ._launch_staged on tables and draws that are already there), timed
            with device events on the engine's stream, table uploads included;
  step      wall time around the whole FlasheCohort.quantize_encrypt (+ sync): draws, tables, allocations, launches.
Per form the median of BLOCKS blocks of REPS runs, with the min - max of the block medians as the spread; `cut` loses a level when
cut / staged - 1 exceeds the larger relative spread of the two.  The sums and the first and last ciphertext of both forms are compared
inside the run.  Shapes: 61,706 x 100 with five scattered clients dropped at int_bits 128 and compact int_bits 23, with twenty dropped in
sixteen runs, batched at int_bits 128 (bs 5) whole and with the five drops; 1e6 x 10 with one client dropped, and batched.
Prints one line per case and level and a final JSON line."""
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flashe_amd import _lib, cipher as cm  # noqa: E402
from flashe_amd.block import FlasheCohort, _cohort_draws  # noqa: E402
from flashe_amd.engine import DeviceVector  # noqa: E402

KEY = bytes(range(32))
BLOCKS, REPS = int(os.environ.get("BLOCKS", "3")), int(os.environ.get("REPS", "5"))
FIVE = (3, 40, 41, 77, 99)
# twenty dropped, the eighty present in sixteen runs: every sixth client from 5 to 77, then 79 .. 81 and 90 .. 93
TWENTY = tuple(range(5, 78, 6)) + (79, 80, 81, 90, 91, 92, 93)
# n, federation, dropped, int_bits, compact, batch
SHAPES = [(61706, 100, FIVE, 128, False, False), (61706, 100, FIVE, 23, True, False), (61706, 100, TWENTY, 128, False, False),
          (61706, 100, (), 128, False, True), (61706, 100, FIVE, 128, False, True),
          (1000000, 10, (4,), 128, False, False), (1000000, 10, (), 128, False, True), (1000000, 10, (4,), 128, False, True)]
cm.N_JOBS = 16


class W:
    def __init__(self, layers):
        self.walking_order = sorted(layers)
        self._weights = dict(layers)


def args(b, eb, batch):
    return {"quantize": {"int_bits": b, "batch": batch, "element_bits": eb, "padding": True, "secure": True}, "precompute": {"enable": False}}


def layer_sizes(n, k=8):
    w = [(i % 7 + 1) ** 3 for i in range(k)]
    sizes = [n * x // (2 * sum(w)) for x in w]
    return sizes + [n - sum(sizes)]


def alternate(forms):
    for fn in forms.values():
        fn()
        fn()                                                   # warm-up of every form
    ms = {f: [] for f in forms}
    for _b in range(BLOCKS):
        for f, fn in forms.items():
            ms[f].append(float(np.median([fn() for _r in range(REPS)])))
    out = {}
    for f, meds in ms.items():
        med = float(np.median(meds))
        out[f] = {"median_ms": med, "min_ms": min(meds), "max_ms": max(meds), "spread": (max(meds) - min(meds)) / med}
    return out


def verdict(row):
    row["staged_over_cut"] = row["staged"]["median_ms"] / row["cut"]["median_ms"]
    row["spread"] = max(row["staged"]["spread"], row["cut"]["spread"])
    row["cut_wins"] = bool(row["staged_over_cut"] - 1.0 > row["spread"])
    row["cut_loses"] = bool(1.0 / row["staged_over_cut"] - 1.0 > row["spread"])
    return row


def timed(eng, fn):
    e0, e1 = eng.event(), eng.event()
    eng.sync()
    eng.record(e0)
    fn()
    eng.record(e1)
    ms = eng.elapsed_ms(e0, e1)
    eng.event_destroy(e0)
    eng.event_destroy(e1)
    return ms


def cohort(b, eb, compact, batch, fed, prefer):
    co = FlasheCohort(args(b, eb, batch), first_idx=0, n_local=fed, num_clients=fed, prp_seed=KEY, compact=compact, cut="any")
    co.set_iter_index(1)
    co.prefer = prefer
    return co


def launch_level(b, eb, compact, batch, fed, present, models):
    """The launches that differ, on one cohort's tables and draws: what quantize_encrypt runs between its draws and its bookkeeping."""
    co = cohort(b, eb, compact, batch, fed, None)
    eng, ld = co.cipher.engine, co.lead
    by_idx = len(present) != fed
    plan, layers, _pre = co._collect([W(dict(m)) for m in models], None, present if by_idx else None)
    assert plan.path == "cut-chain", (plan.path, plan.reason)
    alphas = co._begin_round(plan)
    tables, keep = co._tables(plan, layers, alphas, False)
    C, ne = len(present), plan.n_elems
    np.random.seed(3)
    du = _cohort_draws(eng, C, plan.n, None, None)
    rows = [(st, None, al, sh, _lib.TENSOR_F32, fl) for (st, _p, al, sh, _code, fl) in tables[0]]
    srcs, dts = [[t[1] for t in table] for table in tables], [[t[4] for t in table] for table in tables]

    def vectors():
        if compact:
            return [DeviceVector(eng, ne, 1, elem_bytes=4) for _ in range(C)], DeviceVector(eng, ne, 1, elem_bytes=4)
        return [DeviceVector(eng, ne) for _ in range(C)], DeviceVector(eng, ne)
    (c_cts, c_sum), (s_cts, s_sum) = vectors(), vectors()
    got = {}

    def cut():
        assert co._launch_chain(plan, rows, srcs, dts, du, c_cts, c_sum, by_idx, cut=True), "the cut launch declined the shape"

    def staged():
        got["staged"] = co._launch_staged(plan, tables, du, s_cts, s_sum, False)
    row = alternate({"cut": lambda: timed(eng, cut), "staged": lambda: timed(eng, staged)})
    eng.sync()
    t_cts, t_sum, _held = got["staged"]
    elem = 4 if compact else 16
    for a, s in ((c_sum, t_sum), (c_cts[0], t_cts[0]), (c_cts[-1], t_cts[-1])):
        assert np.array_equal(a.buf.download(np.uint8, elem * ne).copy(), s.buf.download(np.uint8, elem * ne).copy()), "the cut launch differs from the staged form"
    row["parts"], row["runs"], row["n_elems"], row["mask_kept"] = plan.parts, plan.runs, ne, ld._cohort_mask is not None
    del keep
    return row


def step_level(b, eb, compact, batch, fed, present, models):
    cohorts = {"cut": (cohort(b, eb, compact, batch, fed, None), "cut-chain"),
               "staged": (cohort(b, eb, compact, batch, fed, "staged-chain"), "staged-chain")}
    kw = {} if len(present) == fed else {"present": present}

    def run(form):
        co, path = cohorts[form]
        eng = co.cipher.engine
        eng.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        up = co.quantize_encrypt([W(dict(m)) for m in models], **kw)
        eng.sync()
        ms = 1e3 * (time.perf_counter() - t0)
        assert up.path == path, (form, up.path)
        return ms
    return alternate({f: (lambda f=f: run(f)) for f in cohorts})


def main():
    res = {"blocks": BLOCKS, "reps": REPS, "library_sha256_16": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16], "cases": []}
    print(f"n_jobs {cm.N_JOBS}; median of {BLOCKS} blocks of {REPS}, [min - max of the block medians]; baseline: the staged form")
    only = os.environ.get("ONLY")
    for si, (n, fed, dropped, b, compact, batch) in enumerate(SHAPES):
        if only and str(si) not in only.split(","):
            continue
        present = [i for i in range(fed) if i not in dropped]
        eb = min(16, b - (fed - 1).bit_length())
        sizes = layer_sizes(n)
        g = torch.Generator(device="cuda").manual_seed(0)
        models = [{f"l{i:03d}": torch.randn(s, generator=g, device="cuda") * 0.05 + 0.001 * c for i, s in enumerate(sizes)} for c in range(len(present))]
        torch.cuda.synchronize()
        case = {"n": n, "federation": fed, "dropped": len(dropped), "int_bits": b, "compact": compact, "batch": batch, "element_bits": eb}
        tag = f"n {n:>8} x {fed:>3} -{len(dropped):<2} int_bits {b:>3}{' compact' if compact else ''}{' batched' if batch else ''}"
        for name, fn in (("launches", launch_level), ("step", step_level)):
            row = verdict(fn(b, eb, compact, batch, fed, present, models))
            case[name] = row
            print(f"{tag:<44} {name:<8}", " ".join(f"{f} {r['median_ms']:8.3f} ms [{r['min_ms']:.3f} - {r['max_ms']:.3f}]" for f, r in row.items() if isinstance(r, dict)),
                  f"staged/cut {row['staged_over_cut']:.3f} spread {100 * row['spread']:.1f} % cut_wins {row['cut_wins']} cut_loses {row['cut_loses']}"
                  + (f" parts {row['parts']} runs {row['runs']} n_elems {row['n_elems']}" if "parts" in row else ""), flush=True)
        res["cases"].append(case)
        del models
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
