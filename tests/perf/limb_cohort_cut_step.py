#!/usr/bin/env python3
"""The client step of a SHORT one-limb cohort (uint64 ciphertexts, element_bits = int_bits - 8, float32 tensors in nine layers on the GPU):
61,706 values x 100 clients at int_bits 39 and 64, 1e6 x 10 at int_bits 36, and 61,706 x 100 at int_bits 39 with five clients dropped
(six runs of indices).  Two forms of the launches that differ, on draws that are already there, table uploads included, alternated inside
one process after a warm-up and timed with device events on the engine's stream:
  staged   the parent's form for these shapes: a quantise launch per present client into 8-byte plaintexts, then
           flashe_encrypt_batch_sum_dev (C + 2 launches, 36 bytes moved per value and client);
  cut      flashe_quantize_encrypt_cohort_cut_u64_dev: prf_limb_cohort_cut_kernel<3 | 2> over (piece, tile) items and one combine pass.
ALTS alternations (at least seven) give a median per form; `spread` is (max - min) / median of a form's own alternations, and the cut
form `wins` when staged / cut - 1 exceeds the larger of the two spreads.  The two forms' ciphertexts and sums are compared inside the run.
Prints one line per case and a final JSON line."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from flashe_amd import _lib, cipher as cm  # noqa: E402
from flashe_amd.engine import Engine  # noqa: E402

cm.N_JOBS = 16
ALTS = max(7, int(os.environ.get("ALTS", "7")))
KEY = bytes(range(32))
DROPPED = [3, 17, 18, 50, 99]
CASES = [(61706, 100, 39, []), (61706, 100, 64, []), (1000000, 10, 36, []), (61706, 100, 39, DROPPED)]      # n, clients, int_bits, dropped


def timed(eng, fn):
    e0, e1 = eng.event(), eng.event()
    torch.cuda.synchronize()
    eng.record(e0)
    fn()
    eng.record(e1)
    ms = eng.elapsed_ms(e0, e1)
    eng.event_destroy(e0)
    eng.event_destroy(e1)
    return ms


def stats(ms):
    med = float(np.median(ms))
    return {"median_ms": med, "min_ms": float(min(ms)), "max_ms": float(max(ms)), "spread": float((max(ms) - min(ms)) / med)}


def case(n, C, b, dropped):
    eng = Engine(KEY, b, device=0)
    present = [c for c in range(C) if c not in dropped]
    P, EB = len(present), b - 8
    w = [(i % 7 + 1) ** 3 for i in range(8)]
    sizes = [n * x // (2 * sum(w)) for x in w]
    sizes.append(n - sum(sizes))
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    g = torch.Generator(device="cuda").manual_seed(0)
    models = [[torch.randn(s, generator=g, device="cuda") * 0.05 + 0.001 * c for s in sizes] for c in range(P)]
    torch.cuda.synchronize()
    alphas = [0.2 + 0.01 * (i % 5) for i in range(len(sizes))]
    rows = [(starts[i], None, alphas[i], 0.0, _lib.TENSOR_F32, 0) for i in range(len(sizes))]
    srcs = [[t.data_ptr() for t in m] for m in models]
    dts = [[_lib.TENSOR_F32] * len(sizes) for _ in range(P)]
    tables = [[(starts[i], srcs[c][i], alphas[i], 0.0, _lib.TENSOR_F32, 0) for i in range(len(sizes))] for c in range(P)]
    du = eng.alloc(8 * P * n)
    np.random.seed(3)
    eng.numpy_random_dev(P * n, out=du.ptr)
    out = {f: ([eng.alloc_vec(n) for _ in range(P)], eng.alloc_vec(n)) for f in ("staged", "cut")}
    pts = [eng.alloc_vec(n) for _ in range(P)]
    parts = eng.cohort_cut_pieces_u64(present, n, cm.N_JOBS)[0]
    assert parts, "the cut launch declines the shape"
    scratch = eng.alloc(max(8 * parts * n, 16))

    def cut():
        assert eng.quantize_encrypt_cohort_cut_u64_dev(1, present, n, cm.N_JOBS, rows, srcs, dts, EB, du, out["cut"][0], out["cut"][1], scratch)

    def staged():                                              # (FlasheCohort._launch_staged's one-limb form)
        for c in range(P):
            eng.quantize_batch_tensors_dev(tables[c], n, EB, b, du.ptr + 8 * c * n, n, pts[c])
        eng.encrypt_batch_sum_dev(1, present, 1, n, cm.N_JOBS, pts, 1, out["staged"][0], out["staged"][1])

    forms = {"staged": staged, "cut": cut}
    for fn in forms.values():
        fn()                                                   # warm-up of every form
    ms = {f: [] for f in forms}
    for _a in range(ALTS):
        for f, fn in forms.items():
            ms[f].append(timed(eng, fn))
    for a, b_ in zip(out["staged"][0] + [out["staged"][1]], out["cut"][0] + [out["cut"][1]]):
        assert np.array_equal(a.download(np.uint64, n).copy(), b_.download(np.uint64, n)), "the cut launch's bytes differ from the staged form's"
    row = {"n": n, "clients": C, "int_bits": b, "dropped": dropped, "parts": parts, **{f: stats(v) for f, v in ms.items()}}
    row["staged_over_cut"] = row["staged"]["median_ms"] / row["cut"]["median_ms"]
    row["spread"] = max(row["staged"]["spread"], row["cut"]["spread"])
    row["cut_wins"] = bool(row["staged_over_cut"] - 1.0 > row["spread"])
    return row


def main():
    res = {"alternations": ALTS, "library_sha256_16": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16], "cases": []}
    print(f"one limb, element_bits int_bits - 8, n_jobs {cm.N_JOBS}; {ALTS} alternations per form, device events, the launches that differ")
    for n, C, b, dropped in CASES:
        row = case(n, C, b, dropped)
        res["cases"].append(row)
        print(f"n {n:>8} x {C:>3} int_bits {b} dropped {dropped} parts {row['parts']:>2}: " +
              " ".join(f"{f} {row[f]['median_ms']:8.3f} ms [{row[f]['min_ms']:.3f} - {row[f]['max_ms']:.3f}]" for f in ("staged", "cut")) +
              f" staged/cut {row['staged_over_cut']:.3f} spread {100 * row['spread']:.1f} % cut_wins {row['cut_wins']}", flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
