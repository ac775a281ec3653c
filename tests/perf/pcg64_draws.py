#!/usr/bin/env python3
"""The stochastic-rounding draws from a caller's np.random.Generator over PCG64 -- what np.random.default_rng returns -- and PCG64DXSM
(rng=, flashe_pcg64_random_dev: every lane jumps once to its first draw of the 128-bit LCG and walks a fixed stride; one asynchronous
launch for any number of streams) against what the same call cost before: rng.random(n) on one host thread plus an upload of 8 bytes per
draw.  One process, the forms alternated ALTS (at least five) times after a warm-up, timed with device events on the engine's stream
(the host's draws lie between the two events); median [min - max].  In (a) every timed device call follows an untimed call of the same
form: the host form leaves the device idle for a fifth of a second, and the first launch after it would pay for that.
  (a) the generator alone: 1e8 draws as one segment and ten segments of 1e7 draws into one buffer -- host: rng.random + upload_at per
      stretch; pcg64, dxsm: ONE launch; philox: the counter-based launch (flashe_philox_random_dev), for the instruction-mix expectation
      (one 128 x 128 -> 128 low product per draw against five 64 x 64 -> 128 products): read against the store floor, 8 bytes per draw at
      the 6.29 TB/s copy ceiling.  Draws/s and the fraction of the store floor are printed.
  (x) the crossover: at DEVICE_RNG_MIN (65,536) draws, and at 4,096 and 16,384, the host path against the device call by the host clock,
      launch, state hand-back and the wait for the result included -- the device call must not be the slower one at DEVICE_RNG_MIN.
  (b) FlasheCohort.quantize_encrypt as a whole, ten clients of 25,557,032 float32 values held as torch tensors, int_bits 128,
      rng=np.random.default_rng(11): this library against the same call with FLASHE_DEVICE_RNG=0 (the host path).
The first 4,096 draws of every device case are compared with NumPy's own inside the run.  PART=a / x / b runs one part.  Prints one line
per case and a final JSON line."""
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from flashe_amd import _lib, cipher as cm  # noqa: E402
from flashe_amd.engine import Engine  # noqa: E402
from flashe_amd.quantize import DEVICE_RNG_MIN  # noqa: E402

cm.N_JOBS = 16
ALTS = max(5, int(os.environ.get("ALTS", "5")))
PART = os.environ.get("PART", "axb")
LENGTH = int(os.environ.get("LENGTH", "25557032"))
C = 10
KEY = bytes(range(32))
STORE_FLOOR_MS_PER_DRAW = 8 / 6.29e12 * 1e3
BITGENS = {"host": np.random.PCG64, "pcg64": np.random.PCG64, "dxsm": np.random.PCG64DXSM, "philox": np.random.Philox}


def timed(eng, fn):
    e0, e1 = eng.event(), eng.event()
    eng.sync()
    t0 = time.perf_counter()
    eng.record(e0)
    r = fn()
    eng.record(e1)
    ms = eng.elapsed_ms(e0, e1)                                 # (waits for e1)
    wall = (time.perf_counter() - t0) * 1e3
    eng.event_destroy(e0)
    eng.event_destroy(e1)
    return ms, wall, r


def stats(ms):
    med = float(np.median(ms))
    return {"median_ms": med, "min_ms": float(min(ms)), "max_ms": float(max(ms)), "range_ms": float(max(ms) - min(ms))}


def alternate(forms, alts=ALTS):
    for fn in forms.values():
        fn()
    ms = {f: [] for f in forms}
    for _a in range(alts):
        for f, fn in forms.items():
            ms[f].append(fn())
    return {f: {"device": stats([m[0] for m in v]), "wall": stats([m[1] for m in v])} for f, v in ms.items()}


def show(tag, row, forms, clock="device"):
    return tag + " " + " ".join(f"{f} {row[f][clock]['median_ms']:9.3f} ms [{row[f][clock]['min_ms']:.3f} - {row[f][clock]['max_ms']:.3f}]" for f in forms)


def gen(form, seed):
    return np.random.Generator(BITGENS[form](seed))


def draw(eng, form, seeds, n, du):
    """len(seeds) stretches of n draws into du, back to back, the way the form draws them."""
    gens = [gen(form, s) for s in seeds]
    if form == "host":
        for c, g in enumerate(gens):
            du.upload_at(8 * c * n, g.random(n))
    else:
        (eng.philox_random_dev if form == "philox" else eng.pcg64_random_dev)(gens, [n] * len(gens), out=du, offsets=[c * n for c in range(len(gens))])


def part_a(eng, res):
    for n, segments in ((100_000_000, 1), (10_000_000, C)):
        du = eng.alloc(8 * n * segments)
        seeds = [100 + c for c in range(segments)]
        forms = ("host", "pcg64", "dxsm", "philox")

        def one(f):
            if f != "host":                                     # the host form leaves the device idle for its whole length: an untimed call of
                draw(eng, f, seeds, n, du)                      # the same form first, so that every device form starts from a busy device
            return timed(eng, lambda: draw(eng, f, seeds, n, du))[:2]
        row = alternate({f: (lambda f=f: one(f)) for f in forms})
        for f in ("pcg64", "dxsm", "philox"):                   # the last form of a round wrote the buffer: draw once more, and look
            draw(eng, f, seeds, n, du)
            for c in (0, segments - 1):
                assert du.download_at(8 * c * n, np.float64, 4096).tobytes() == gen(f, seeds[c]).random(4096).tobytes(), f"{f}: the device draws differ from NumPy's"
        total = n * segments
        for f in forms[1:]:
            med = row[f]["device"]["median_ms"]
            row[f].update(gdraws_per_s=total / med / 1e6, over_store_floor=med / (total * STORE_FLOOR_MS_PER_DRAW))
        row.update(n=n, segments=segments, host_over_pcg64=row["host"]["device"]["median_ms"] / row["pcg64"]["device"]["median_ms"],
                   pcg64_over_philox=row["pcg64"]["device"]["median_ms"] / row["philox"]["device"]["median_ms"])
        res["generator"].append(row)
        print(show(f"(a) {segments:>2} x {n:>9} draws", row, forms), flush=True)
        print("    " + "; ".join(f"{f} {row[f]['gdraws_per_s']:.1f} G draws/s, {row[f]['over_store_floor']:.2f} x the store floor" for f in forms[1:])
              + f"; host / pcg64 {row['host_over_pcg64']:.0f}, pcg64 / philox {row['pcg64_over_philox']:.2f}", flush=True)
        du.free()


def part_x(eng, res):
    for n in (4096, 16384, DEVICE_RNG_MIN):
        du = eng.alloc(8 * n)
        forms = ("host", "pcg64", "dxsm")
        row = alternate({f: (lambda f=f: timed(eng, lambda: draw(eng, f, [7], n, du))[:2]) for f in forms}, alts=max(ALTS, 25))
        row.update(n=n, device_not_slower=bool(row["pcg64"]["wall"]["median_ms"] <= row["host"]["wall"]["median_ms"]
                                               and row["dxsm"]["wall"]["median_ms"] <= row["host"]["wall"]["median_ms"]))
        res["crossover"].append(row)
        print(show(f"(x) {n:>6} draws, host clock", row, forms, "wall"), f"device not slower: {row['device_not_slower']}", flush=True)
        du.free()


class W:
    def __init__(self, layers):
        self.walking_order = sorted(layers)
        self._weights = dict(layers)


def layer_sizes(n, k=40):
    w = [(i % 7 + 1) ** 3 for i in range(k)]
    sizes = [n * x // (2 * sum(w)) for x in w]
    return sizes + [n - sum(sizes)]


def part_b(res):
    import torch
    from flashe_amd.block import FlasheCohort
    n = LENGTH
    sizes = layer_sizes(n)
    g = torch.Generator(device="cuda").manual_seed(0)
    models = [{f"l{i:03d}": torch.randn(s, generator=g, device="cuda") * 0.05 + 0.001 * c for i, s in enumerate(sizes)} for c in range(C)]
    torch.cuda.synchronize()
    args = {"quantize": {"int_bits": 128, "batch": False, "element_bits": 16, "padding": True, "secure": True}, "precompute": {"enable": False}}
    cohorts = {f: FlasheCohort(args, first_idx=0, n_local=C, num_clients=C, prp_seed=KEY) for f in ("host", "device")}
    paths, sums = {}, {}

    def run(form):
        co = cohorts[form]
        co.set_iter_index(1)
        os.environ["FLASHE_DEVICE_RNG"] = "0" if form == "host" else "1"
        try:
            ms, wall, up = timed(co.cipher.engine, lambda: co.quantize_encrypt([W(dict(m)) for m in models], rng=np.random.default_rng(11)))
        finally:
            os.environ.pop("FLASHE_DEVICE_RNG")
        paths[form] = up.path
        if form not in sums:                                    # (the warm-up round: outside the timed rounds' rhythm)
            sums[form] = hashlib.sha256(up.partial_sum.to_host().tobytes()).hexdigest()[:16]
        return ms, wall
    row = alternate({f: (lambda f=f: run(f)) for f in cohorts})
    assert sums["host"] == sums["device"], "the two forms' partial sums differ"
    row.update(n=n, int_bits=128, paths=paths, host_over_device=row["host"]["device"]["median_ms"] / row["device"]["device"]["median_ms"])
    res["cohort_step"].append(row)
    print(show(f"(b) {C} clients x {n} values, int_bits 128 ({paths['device']}), rng=default_rng(11)", row, ("host", "device")),
          f"host / device {row['host_over_device']:.1f}", flush=True)


def main():
    res = {"alternations": ALTS, "library_sha256_16": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16], "generator": [],
           "crossover": [], "cohort_step": []}
    print(f"{ALTS} alternations per form, device events around the call (host draws and uploads lie between them)")
    if "b" in PART:
        import torch                  # (before the first engine: the framework then still finds its device)
        torch.zeros(1, device="cuda")
        torch.cuda.synchronize()
    eng = Engine(KEY, 128, device=0)
    if "a" in PART:
        part_a(eng, res)
    if "x" in PART:
        part_x(eng, res)
    if "b" in PART:
        part_b(res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
