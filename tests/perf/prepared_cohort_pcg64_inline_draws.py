#!/usr/bin/env python3
"""The online launch of a precompute job's cohort (ten co-located clients, float32 models of 1e7 and of 25,557,032 values) with the
stochastic-rounding draws of np.random.default_rng's generators (PCG64) and of np.random.PCG64DXSM ones, two forms alternated inside one
process after a warm-up and timed with device events on the engine's stream, table uploads included:
  A  the draws materialised first: pcg64_random_dev (one launch, 8 bytes written per value and client) + quantize_combine_cohort_dev
     (which reads them back) -- the round as it runs without inline_draws="any";
  B  quantize_combine_cohort_pcg64_dev: the one launch generates them, no draw buffer.
At int_bits 128 (two limbs: 36 bytes per value and client without the draws) and at int_bits 20 compact (12 bytes), each from
  shared  one generator for all clients that has drawn one value: client c's stretch starts 1 + c n draws in;
  list    one fresh generator per client.
Both forms start every run from equal generator states; their ciphertexts and sums are compared inside the run.  ALTS alternations (at
least seven) give a median per form; `spread` is (max - min) / median of a form's own alternations and B `wins` a case when A / B - 1
exceeds the larger of the two spreads.  A layout (compact or not) -- the key of flashe_amd.block._INLINE_PCG64_DEFAULT -- becomes inline
by default only where B wins EVERY case of it.  Prints one line per case, one per layout and a final JSON line."""
import copy
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from flashe_amd import _lib  # noqa: E402
from flashe_amd.engine import Engine  # noqa: E402

C = int(os.environ.get("CLIENTS", "10"))
ALTS = max(7, int(os.environ.get("ALTS", "7")))
LENGTHS = [int(v) for v in os.environ.get("LENGTHS", "10000000,25557032").split(",")]
SETTINGS = [(128, False), (20, True)]                                  # int_bits, compact
VARIANTS = ["PCG64", "PCG64DXSM"]
KEY = bytes(range(32))
EB, N_JOBS = 16, 16
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


def generators(variant, shared):
    kind = getattr(np.random, variant)
    if not shared:
        return [np.random.Generator(kind(100 + c)) for c in range(C)]
    g = np.random.Generator(kind(99))
    g.random(1)
    return g


def table(rng, n):
    return (rng, [n] * C, [c * n for c in range(C)]) if isinstance(rng, list) else ([rng], [C * n], [0])


def case(eng, compact, n, variant, shared, xs, masks):
    L = eng.limbs
    sizes = layer_sizes(n)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    alphas = [0.2 + 0.01 * (i % 5) for i in range(len(sizes))]
    rows = [(starts[i], None, alphas[i], 0.0, _lib.TENSOR_F32, 0) for i in range(len(sizes))]
    srcs = [[x.ptr + 4 * s for s in starts] for x in xs]
    dts = [[_lib.TENSOR_F32] * len(sizes) for _ in range(C)]
    elem = 4 if compact else 8 * L
    du = eng.alloc(8 * C * n)
    out = {f: ([eng.alloc(elem * n) for _ in range(C)], eng.alloc(elem * n)) for f in "AB"}
    start = generators(variant, shared)

    def form_a(rng):
        gens, counts, offsets = table(rng, n)
        eng.pcg64_random_dev(gens, counts, out=du, offsets=offsets)
        assert eng.quantize_combine_cohort_dev(n, rows, srcs, dts, EB, du, masks, out["A"][0], out["A"][1], compact=compact)

    def form_b(rng):
        gens, counts, offsets = table(rng, n)
        assert eng.quantize_combine_cohort_pcg64_dev(n, rows, srcs, dts, EB, gens, counts, offsets, masks, out["B"][0], out["B"][1], compact=compact)

    forms = {"A": form_a, "B": form_b}
    ends = {}
    for f, fn in forms.items():                                        # warm-up of every form, and the parity of what they wrote
        rng = copy.deepcopy(start)
        fn(rng)
        ends[f] = rng
    eng.sync()
    some = sorted({0, C // 2, C - 1})                                  # (the sum and three clients' ciphertexts: the downloads are not free)
    for va, vb in zip([out["A"][0][c] for c in some] + [out["A"][1]], [out["B"][0][c] for c in some] + [out["B"][1]]):
        a, b = (v.download(np.uint32, n * elem // 4).copy() for v in (va, vb))
        assert np.array_equal(a, b), "the inline form's ciphertexts or sum differ from the buffer form's"
    for ga, gb in zip(*([ends["A"]], [ends["B"]]) if shared else (ends["A"], ends["B"])):
        assert ga.bit_generator.state == gb.bit_generator.state, "the two forms leave the generators in different states"
    ms = {f: [] for f in forms}
    for _a in range(ALTS):
        for f, fn in forms.items():
            rng = copy.deepcopy(start)
            ms[f].append(timed(eng, lambda: fn(rng)))
    row = {f: stats(v) for f, v in ms.items()}
    row["A_over_B"] = row["A"]["median_ms"] / row["B"]["median_ms"]
    row["spread"] = max(row["A"]["spread"], row["B"]["spread"])
    row["B_wins"] = bool(row["A_over_B"] - 1.0 > row["spread"])
    # what each form must move per value and client: the float, the mask, the ciphertext (+ the sum once); A also writes and reads a draw
    moved_b = C * n * (4 + 2 * elem) + elem * n
    row["bytes"] = {"A": moved_b + 16 * C * n, "B": moved_b}
    row["B_TBps"] = moved_b / (row["B"]["median_ms"] * 1e-3) / 1e12
    row["B_of_copy_ceiling"] = row["B_TBps"] * 1e12 / COPY_CEILING
    row["B_draws_per_s"] = C * n / (row["B"]["median_ms"] * 1e-3)
    return row


def main():
    res = {"clients": C, "alternations": ALTS, "library": os.path.basename(_lib.LIB_PATH),
           "library_sha256_16": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16], "cases": []}
    print(f"{C} clients, element_bits {EB}; {ALTS} alternations per form, device events on one stream; {res['library']}", flush=True)
    for n in LENGTHS:
        for b, compact in SETTINGS:
            eng = Engine(KEY, b, device=0)
            print(f"the launch's grid for n {n}: {eng.pcg64_cohort_grid(n)} workgroups", flush=True)
            r = np.random.Generator(np.random.PCG64(n))
            base = (r.standard_normal(n, dtype=np.float32) * np.float32(0.05))
            xs = [eng.upload(base + np.float32(0.001 * c)) for c in range(C)]
            masks = [eng.alloc((4 if compact else 8 * eng.limbs) * n) for _ in range(C)]
            eng.cohort_masks_dev(2, 0, C, n, N_JOBS, masks, compact=compact)
            for variant in VARIANTS:
                for shared in (True, False):
                    row = case(eng, compact, n, variant, shared, xs, masks)
                    row.update({"n": n, "int_bits": b, "compact": compact, "variant": variant, "shared": shared})
                    res["cases"].append(row)
                    print(f"n {n:>9} int_bits {b:>3}{' compact' if compact else '        '} {variant:<9} {'shared' if shared else 'list  '} " +
                          " ".join(f"{f} {row[f]['median_ms']:8.3f} ms [{row[f]['min_ms']:.3f} .. {row[f]['max_ms']:.3f}]" for f in "AB") +
                          f" A/B {row['A_over_B']:.3f} spread {100 * row['spread']:.1f} % B_wins {row['B_wins']}; B {row['B_TBps']:.2f} TB/s = "
                          f"{100 * row['B_of_copy_ceiling']:.0f} % of the copy ceiling, {row['B_draws_per_s']:.2e} draws/s", flush=True)
            del xs, masks
            eng.close()
    res["layout_default"] = {}
    for compact in (False, True):
        mine = [row for row in res["cases"] if row["compact"] == compact]
        res["layout_default"]["compact" if compact else "limbs"] = all(row["B_wins"] for row in mine)
        print(f"layout {'compact' if compact else 'limbs  '}: B wins {sum(row['B_wins'] for row in mine)} of {len(mine)} cases -> "
              f"_INLINE_PCG64_DEFAULT[{compact}] = {res['layout_default']['compact' if compact else 'limbs']}", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
