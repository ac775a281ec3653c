#!/usr/bin/env python3
"""The online launch of a BATCHED precompute job's cohort (co-located clients, float32 models) with the stochastic-rounding draws of
np.random.Philox generators, two forms alternated inside one process after settle rounds and timed with device events on the engine's
stream, table uploads included:
  A  the draws materialised first: philox_random_dev (one launch, 8 bytes written per value and client) +
     quantize_combine_cohort_dev(batch=...) (which reads them back) -- the code of the commit before the inline form, untouched by it;
  B  quantize_combine_cohort_philox_dev(batch=...): the one launch generates them, no draw buffer; a lane owns four elements.
Shapes: ten clients at 25,557,032 and 1e7 values, int_bits 120 (six values per element) and int_bits 128 with 18-bit fields (seven),
and 100 clients of 61,706 values at int_bits 120 (five), each
  aligned     one fresh generator per client: every client's stream starts at a block;
  misaligned  one shared generator that has drawn one value, over models of n + 1 values: the clients' phases differ.
Both forms start every run from equal generator states; their ciphertexts and sums are compared inside the run.  ALTS alternations (at
least seven) give a median per form; `spread` is (max - min) / median of a form's own alternations and B `wins` a class (values per
element x alignment) when A / B - 1 exceeds the larger of the two spreads in EVERY shape of the class -- the rule by which the inline
form becomes that class's default in flashe_amd.block._INLINE_BATCHED_DEFAULT.  Prints one line per case and a final JSON line."""
import copy
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from flashe_amd import _lib  # noqa: E402
from flashe_amd.engine import Engine  # noqa: E402

ALTS = max(7, int(os.environ.get("ALTS", "7")))
SETTLE = int(os.environ.get("SETTLE", "2"))
# clients, values, int_bits, element_bits, field_bits = element_bits + ceil(log2 clients)
SHAPES = [(10, 25557032, 120, 16, 20), (10, 25557032, 128, 14, 18), (10, 10000000, 120, 16, 20), (10, 10000000, 128, 14, 18), (100, 61706, 120, 16, 23)]
KEY = bytes(range(32))
N_JOBS = 16
COPY_CEILING = 6.29e12


def layer_sizes(n, k=40):
    w = [(i % 7 + 1) ** 3 for i in range(k)]
    sizes = [n * x // (2 * sum(w)) for x in w]
    return sizes + [n - sum(sizes)]


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


def stats(ms):
    med = float(np.median(ms))
    return {"median_ms": med, "min_ms": float(min(ms)), "max_ms": float(max(ms)), "spread": float((max(ms) - min(ms)) / med)}


def generators(C, aligned):
    if aligned:
        return [np.random.Generator(np.random.Philox(100 + c)) for c in range(C)]
    g = np.random.Generator(np.random.Philox(99))
    g.random(1)
    return g


def table(rng, C, n):
    return (rng, [n] * C, [c * n for c in range(C)]) if isinstance(rng, list) else ([rng], [C * n], [0])


def case(eng, C, n, eb, fb, aligned, xs):
    L = eng.limbs
    bs = eng.int_bits // fb
    sizes = layer_sizes(n)
    n_elems = sum(-(-s // bs) for s in sizes)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    alphas = [0.2 + 0.01 * (i % 5) for i in range(len(sizes))]
    rows = [(starts[i], None, alphas[i], 0.0, _lib.TENSOR_F32, 0) for i in range(len(sizes))]
    srcs = [[x.ptr + 4 * s for s in starts] for x in xs]
    dts = [[_lib.TENSOR_F32] * len(sizes) for _ in range(C)]
    elem = 8 * L
    masks = [eng.alloc(elem * n_elems) for _ in range(C)]
    eng.cohort_masks_dev(2, 0, C, n_elems, N_JOBS, masks)
    du = eng.alloc(8 * C * n)
    out = {f: ([eng.alloc(elem * n_elems) for _ in range(C)], eng.alloc(elem * n_elems)) for f in "AB"}
    start = generators(C, aligned)

    def form_a(rng):
        gens, counts, offsets = table(rng, C, n)
        eng.philox_random_dev(gens, counts, out=du, offsets=offsets)
        assert eng.quantize_combine_cohort_dev(n, rows, srcs, dts, eb, du, masks, out["A"][0], out["A"][1], batch=(n_elems, fb))

    def form_b(rng):
        gens, counts, offsets = table(rng, C, n)
        assert eng.quantize_combine_cohort_philox_dev(n, rows, srcs, dts, eb, gens, counts, offsets, masks, out["B"][0], out["B"][1], batch=(n_elems, fb))

    forms = {"A": form_a, "B": form_b}
    ends = {}
    for _s in range(max(1, SETTLE)):                                   # settle rounds of every form, and the parity of what they wrote
        for f, fn in forms.items():
            rng = copy.deepcopy(start)
            fn(rng)
            ends[f] = rng
    eng.sync()
    some = sorted({0, C // 2, C - 1})                                  # (the sum and three clients' ciphertexts: the downloads are not free)
    for va, vb in zip([out["A"][0][c] for c in some] + [out["A"][1]], [out["B"][0][c] for c in some] + [out["B"][1]]):
        a, b = (v.download(np.uint32, n_elems * elem // 4).copy() for v in (va, vb))
        assert np.array_equal(a, b), "the inline form's ciphertexts or sum differ from the buffer form's"
    for ga, gb in zip(*(ends["A"], ends["B"]) if aligned else ([ends["A"]], [ends["B"]])):
        assert np.array_equal(ga.random(4), gb.random(4)), "the two forms leave the generators at different positions"
    ms = {f: [] for f in forms}
    for _a in range(ALTS):
        for f, fn in forms.items():
            rng = copy.deepcopy(start)
            ms[f].append(timed(eng, lambda: fn(rng)))
    row = {f: stats(v) for f, v in ms.items()}
    row["A_over_B"] = row["A"]["median_ms"] / row["B"]["median_ms"]
    row["spread"] = max(row["A"]["spread"], row["B"]["spread"])
    row["B_wins"] = bool(row["A_over_B"] - 1.0 > row["spread"])
    # what each form must move: per value and client the float, per element and client the mask and the ciphertext (+ the sum once); A
    # also writes and reads a draw per value and client
    moved_b = C * (4 * n + 2 * elem * n_elems) + elem * n_elems
    row["bytes"] = {"A": moved_b + 16 * C * n, "B": moved_b}
    row["B_TBps"] = moved_b / (row["B"]["median_ms"] * 1e-3) / 1e12
    row["B_of_copy_ceiling"] = row["B_TBps"] * 1e12 / COPY_CEILING
    row["B_draws_per_s"] = C * n / (row["B"]["median_ms"] * 1e-3)
    row.update({"bs": bs, "n_elems": n_elems})
    return row


def main():
    res = {"alternations": ALTS, "settle": SETTLE, "library": os.path.basename(_lib.LIB_PATH),
           "library_sha256_16": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16], "cases": []}
    print(f"{ALTS} alternations per form after {SETTLE} settle rounds, device events on one stream; {res['library']}", flush=True)
    for C, n0, b, eb, fb in SHAPES:
        eng = Engine(KEY, b, device=0)
        r = np.random.Generator(np.random.PCG64(n0))
        base = (r.standard_normal(n0 + 1, dtype=np.float32) * np.float32(0.05))
        xs = [eng.upload(base + np.float32(0.001 * c)) for c in range(C)]
        for aligned in (True, False):
            n = n0 if aligned else n0 + 1
            row = case(eng, C, n, eb, fb, aligned, xs)
            row.update({"clients": C, "n": n, "int_bits": b, "field_bits": fb, "aligned": aligned})
            res["cases"].append(row)
            print(f"C {C:>3} n {n:>9} int_bits {b:>3} bs {row['bs']} {'aligned   ' if aligned else 'misaligned'} " +
                  " ".join(f"{f} {row[f]['median_ms']:8.3f} ms [{row[f]['min_ms']:.3f} .. {row[f]['max_ms']:.3f}]" for f in "AB") +
                  f" A/B {row['A_over_B']:.3f} spread {100 * row['spread']:.1f} % B_wins {row['B_wins']}; B {row['B_TBps']:.2f} TB/s = "
                  f"{100 * row['B_of_copy_ceiling']:.0f} % of the copy ceiling, {row['B_draws_per_s']:.2e} draws/s", flush=True)
        del xs
        eng.close()
    classes = {}
    for row in res["cases"]:
        classes.setdefault((row["bs"], row["aligned"]), []).append(row["B_wins"])
    res["classes"] = [{"bs": bs, "aligned": al, "B_wins_every_shape": all(v)} for (bs, al), v in sorted(classes.items())]
    for cl in res["classes"]:
        print(f"class bs {cl['bs']} {'aligned' if cl['aligned'] else 'misaligned'}: inline wins every shape: {cl['B_wins_every_shape']}", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
