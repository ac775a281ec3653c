#!/usr/bin/env python3
"""A precompute job's cohort of ten co-located clients, models of 1e7 and of 25,557,032 float32 values held as torch tensors on the GPU,
at int_bits 20 in the compact layout and at int_bits 120 batched (element_bits 16).  Two forms, alternated inside one process after a
warm-up, every engine on ONE stream and timed with device events on it:
  A  the parent's form: every client its own masks (FlasheClient.prepare_encrypt: 2 C streams, 2 C one-limb vectors in HBM) and its own
     prepared step, then the aggregate and -- compact -- the narrowing (FlasheCohort's `_clients` path, "per-client");
  B  the cohort's form: FlasheCohort.prepare_encrypt (one chain of C + 1 streams, C vectors) and ONE online launch ("prepared-cohort").
Levels:
  masks     the idle-time mask cost;
  launches  the online launches that differ, on draws and masks that are already there (A: C x quantize_(batch_)encrypt_prepared_tensors_dev
            + aggregate_elem_dev (+ C + 1 narrow_u32_dev); B: quantize_combine_cohort_dev), table uploads included; B's achieved
            bytes per second over the bytes it must move, against the 6.29 TB/s copy ceiling of NOTES section 4;
  step      FlasheCohort.quantize_encrypt as a whole (the draws of all clients are generated inside it, alike in both forms).
ALTS alternations (at least seven) give a median per form; `spread` is (max - min) / median of a form's own alternations, and B `wins`
a level when A / B - 1 exceeds the larger of the two spreads.  With FLASHE_LIB_NAME=libflashe_hip_tuning.so the client-group size of B's
kernel (FLASHE_PREP_COHORT_GROUP = 1 / 2 / 4) is alternated the same way at the launch level, and only that level runs.  Prints one line
per case and level and a final JSON line."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from flashe_amd import _lib, cipher as cm  # noqa: E402
from flashe_amd.block import FlasheCohort  # noqa: E402
from flashe_amd.engine import Engine  # noqa: E402


class W:
    def __init__(self, layers):
        self.walking_order = sorted(layers)
        self._weights = dict(layers)


cm.N_JOBS = 16
C = int(os.environ.get("CLIENTS", "10"))
ALTS = max(7, int(os.environ.get("ALTS", "7")))
LENGTHS = [int(v) for v in os.environ.get("LENGTHS", "10000000,25557032").split(",")]
SETTINGS = [(20, False, True), (120, True, False)]                     # int_bits, batched, compact
KEY = bytes(range(32))
EB = 16
COPY_CEILING = 6.29e12
TUNING = "tuning" in os.path.basename(_lib.LIB_PATH)


def layer_sizes(n, k=40):
    w = [(i % 7 + 1) ** 3 for i in range(k)]
    sizes = [n * x // (2 * sum(w)) for x in w]
    return sizes + [n - sum(sizes)]


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
    a, b = row["A"], row["B"]
    row["A_over_B"] = a["median_ms"] / b["median_ms"]
    row["spread"] = max(a["spread"], b["spread"])
    row["B_wins"] = bool(row["A_over_B"] - 1.0 > row["spread"])
    return row


def alternate(forms, before=None):
    """before[f]: what a form needs ahead of every timed run (its masks), not timed"""
    before = before or {}
    for f, fn in forms.items():
        before.get(f, lambda: None)()
        fn()                                                       # warm-up of every form
    ms = {f: [] for f in forms}
    for _a in range(ALTS):
        for f, fn in forms.items():
            before.get(f, lambda: None)()
            ms[f].append(fn())
    return {f: stats(v) for f, v in ms.items()}


def n_elems_of(sizes, b, batched):
    if not batched:
        return sum(sizes)
    bs = b // (EB + int(np.ceil(np.log2(C))))
    return sum((s + bs - 1) // bs for s in sizes)


def class_levels(b, batched, compact, models, sizes, stream):
    """masks and step through FlasheCohort: A = a cohort whose clients prepare on their own, B = a cohort that prepares as one."""
    n_ct = n_elems_of(sizes, b, batched)
    args = {"quantize": {"int_bits": b, "batch": batched, "element_bits": EB, "padding": True, "secure": True},
            "precompute": {"enable": True, "num_params": n_ct}}
    co = {f: FlasheCohort(args, first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, compact=compact, stream=stream) for f in ("A", "B")}
    for c in co.values():
        c.set_iter_index(1)

    def prep_a():
        for cl in co["A"]._clients:
            cl.prepare_encrypt()

    prep = {"A": prep_a, "B": co["B"].prepare_encrypt}
    masks = alternate({f: (lambda f=f: timed(co[f].cipher.engine, prep[f])[0]) for f in co})

    def run(f):
        ms, up = timed(co[f].cipher.engine, lambda: co[f].quantize_encrypt([W(dict(m)) for m in models]))
        assert up.path == ("per-client" if f == "A" else "prepared-cohort"), (f, up.path)
        return ms, up
    step = alternate({f: (lambda f=f: run(f)[0]) for f in co}, before=prep)
    # the two forms computed the same values
    np.random.seed(5)
    prep["A"]()
    ua = run("A")[1]
    np.random.seed(5)
    prep["B"]()
    ub = run("B")[1]
    sa, sb = ua.partial_sum.to_host(), ub.partial_sum.to_host()
    assert sa.dtype == sb.dtype and np.array_equal(sa, sb), "the cohort's sum differs from the clients' own"
    elem = 4 if compact else 8 * co["B"].cipher.engine.limbs
    held = {"A": 2 * C * n_ct * 8 * co["A"].cipher.engine.limbs, "B": C * n_ct * elem}
    return masks, step, held


def launch_level(b, batched, compact, models, sizes, stream):
    engs = [Engine(KEY, b, device=0, stream=stream) for _ in range(C)]
    eng = engs[0]
    L = eng.limbs
    n, n_ct = sum(sizes), n_elems_of(sizes, b, batched)
    fb = EB + int(np.ceil(np.log2(C)))
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
    elem = 4 if compact else 8 * L
    masks = [eng.alloc(elem * n_ct) for _ in range(C)]
    eng.cohort_masks_dev(2, 0, C, n_ct, cm.N_JOBS, masks, compact=compact)
    cts_b, sum_b = [eng.alloc(elem * n_ct) for _ in range(C)], eng.alloc(elem * n_ct)
    cts_a, sum_a = [eng.alloc_vec(n_ct) for _ in range(C)], eng.alloc_vec(n_ct)
    cts_a32, sum_a32 = ([eng.alloc(4 * n_ct) for _ in range(C)], eng.alloc(4 * n_ct)) if compact else (None, None)

    def prep_a():
        for c in range(C):
            engs[c].prepare_encrypt(2, c, 1, n_ct, cm.N_JOBS)

    def form_a():
        for c in range(C):
            if batched:
                engs[c].quantize_batch_encrypt_prepared_tensors_dev(tables[c], n, EB, fb, du.ptr + 8 * c * n, n_ct, cts_a[c])
            else:
                engs[c].quantize_encrypt_prepared_tensors_dev(n, 0, n, tables[c], EB, du.ptr + 8 * c * n, cts_a[c])
        eng.aggregate_elem_dev(cts_a, n_ct, sum_a)
        if compact:
            for c in range(C):
                eng.narrow_u32_dev(n_ct, cts_a[c], cts_a32[c])
            eng.narrow_u32_dev(n_ct, sum_a, sum_a32)

    def form_b():
        assert eng.quantize_combine_cohort_dev(n, rows, srcs, dts, EB, du, masks, cts_b, sum_b, compact=compact, batch=(n_ct, fb) if batched else None)

    res = alternate({"A": lambda: timed(eng, form_a)[0], "B": lambda: timed(eng, form_b)[0]}, before={"A": prep_a})
    got_a = (sum_a32.download(np.uint32, n_ct) if compact else sum_a.download(np.uint64, n_ct * L)).copy()
    got_b = (sum_b.download(np.uint32, n_ct) if compact else sum_b.download(np.uint64, n_ct * L)).copy()
    assert np.array_equal(got_a, got_b), "the one launch's sum differs from the clients' own steps'"
    # what B must move: per client the floats, the draws, the mask and the ciphertext; the sum once
    moved = C * (4 * n + 8 * n + 2 * elem * n_ct) + elem * n_ct
    res["B_bytes"] = moved
    res["B_bytes_per_value_and_client"] = moved / (C * n)
    res["B_TBps"] = moved / (res["B"]["median_ms"] * 1e-3) / 1e12
    res["B_of_copy_ceiling"] = moved / (res["B"]["median_ms"] * 1e-3) / COPY_CEILING
    groups = None
    if TUNING:
        def grouped(g):
            os.environ["FLASHE_PREP_COHORT_GROUP"] = str(g)
            ms = timed(eng, form_b)[0]
            del os.environ["FLASHE_PREP_COHORT_GROUP"]
            return ms
        groups = alternate({f"G{g}": (lambda g=g: grouped(g)) for g in (1, 2, 4)})
    return res, groups


def main():
    res = {"clients": C, "alternations": ALTS, "library": os.path.basename(_lib.LIB_PATH),
           "library_sha256_16": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16], "cases": []}
    print(f"{C} clients, element_bits {EB}, n_jobs {cm.N_JOBS}; {ALTS} alternations per form, device events on one stream; {res['library']}")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for n in LENGTHS:
            sizes = layer_sizes(n)
            g = torch.Generator(device="cuda").manual_seed(0)
            models = [{f"l{i:03d}": torch.randn(s, generator=g, device="cuda") * 0.05 + 0.001 * c for i, s in enumerate(sizes)} for c in range(C)]
            torch.cuda.synchronize()
            for b, batched, compact in SETTINGS:
                case = {"n": n, "int_bits": b, "batched": batched, "compact": compact}
                launches, groups = launch_level(b, batched, compact, models, sizes, stream.cuda_stream)
                torch.cuda.empty_cache()
                tag = f"n {n:>9} int_bits {b}{' batched' if batched else ''}{' compact' if compact else ''}"
                levels = [("launches", launches)]
                held = None
                if not TUNING:
                    masks, step, held = class_levels(b, batched, compact, models, sizes, stream.cuda_stream)
                    case["mask_bytes_held"] = held
                    levels = [("masks", masks), ("launches", launches), ("step", step)]
                for name, row in levels:
                    verdict(row)
                    case[name] = row
                    print(f"{tag} {name:<8}", " ".join(f"{f} {row[f]['median_ms']:8.3f} ms [{row[f]['min_ms']:.3f} - {row[f]['max_ms']:.3f}]" for f in ("A", "B")),
                          f"A/B {row['A_over_B']:.3f} spread {100 * row['spread']:.1f} % B_wins {row['B_wins']}", flush=True)
                print(f"{tag} B moves {launches['B_bytes_per_value_and_client']:.1f} B per value and client: {launches['B_TBps']:.2f} TB/s = "
                      f"{100 * launches['B_of_copy_ceiling']:.0f} % of the 6.29 TB/s copy ceiling" +
                      (f"; masks held A {held['A'] / 1e9:.2f} GB, B {held['B'] / 1e9:.2f} GB" if held else ""), flush=True)
                if groups:
                    case["groups"] = groups
                    print(f"{tag} group   ", " ".join(f"{f} {r['median_ms']:8.3f} ms [{r['min_ms']:.3f} - {r['max_ms']:.3f}]" for f, r in groups.items()), flush=True)
                res["cases"].append(case)
                torch.cuda.empty_cache()
            del models
    print(json.dumps(res))


if __name__ == "__main__":
    main()
