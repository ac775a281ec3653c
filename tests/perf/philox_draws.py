#!/usr/bin/env python3
"""The stochastic-rounding draws from a caller's np.random.Generator over Philox (rng=, flashe_philox_random_dev: counter based, one
asynchronous launch for any number of streams) against the draws of NumPy's global MT19937 stream (flashe_mt19937_random_dev: jump-ahead
trees, one twist wave per substream, synchronous).  One process, the two forms alternated ALTS (at least nine) times after a warm-up,
timed with device events on the engine's stream; median [min - max].
  (a) the generator alone: 1e7, 1e8 and 2.56e8 draws into one buffer (the MT19937 form in calls of at most 2^26 draws, as block.py makes
      them), and ten seeded per-client stretches of 1e7 draws -- ten np.random.seed + device calls against ONE launch of ten segments.
      Philox `wins` when the MT19937 median exceeds its median by more than the two forms' (max - min) ranges combined.  Read against the
      store floor (8 bytes per draw at the 6.29 TB/s copy ceiling: 0.127 ms per 1e8 draws) and the multiply work (20 64 x 64 -> 128
      products per four draws): draws/s and the fraction of the store floor are printed.
  (b) FlasheCohort.quantize_encrypt as a whole, ten clients, models of 1e7 and 25,557,032 float32 values held as torch tensors, int_bits
      128 and 20 compact: rng=Generator(Philox) against rng=None.  A difference inside the larger spread is reported as no gain.
The first 4,096 draws of every Philox case are compared with NumPy's own inside the run.  PART=a / PART=b runs one part.  Prints one line
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

cm.N_JOBS = 16
ALTS = max(9, int(os.environ.get("ALTS", "9")))
PART = os.environ.get("PART", "ab")
COUNTS = [int(float(v)) for v in os.environ.get("COUNTS", "1e7,1e8,2.56e8").split(",")]
LENGTHS = [int(v) for v in os.environ.get("LENGTHS", "10000000,25557032").split(",")]
C = 10
KEY = bytes(range(32))
RUN_MAX = 1 << 26
STORE_FLOOR_MS_PER_DRAW = 8 / 6.29e12 * 1e3


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


def alternate(forms):
    for fn in forms.values():
        fn()
    ms = {f: [] for f in forms}
    for _a in range(ALTS):
        for f, fn in forms.items():
            ms[f].append(fn())
    return {f: {"device": stats([m[0] for m in v]), "wall": stats([m[1] for m in v])} for f, v in ms.items()}


def verdict(row, a="mt19937", b="philox"):
    da, db = row[a]["device"], row[b]["device"]
    row["ratio"] = da["median_ms"] / db["median_ms"]
    row["philox_wins"] = bool(da["median_ms"] - db["median_ms"] > da["range_ms"] + db["range_ms"])
    return row


def show(tag, row, forms):
    return tag + " " + " ".join(f"{f} {row[f]['device']['median_ms']:8.3f} ms [{row[f]['device']['min_ms']:.3f} - {row[f]['device']['max_ms']:.3f}]"
                                f" (wall {row[f]['wall']['median_ms']:.3f})" for f in forms)


def philox(seed):
    return np.random.Generator(np.random.Philox(seed))


def check_head(buf, seed, at=0):
    got = buf.download_at(8 * at, np.float64, 4096)
    assert got.tobytes() == philox(seed).random(4096).tobytes(), "the device draws differ from NumPy's"


def part_a(eng, res):
    for n in COUNTS:
        du = eng.alloc(8 * n)

        def mt():
            np.random.seed(5)
            for at in range(0, n, RUN_MAX):
                eng.numpy_random_dev(min(RUN_MAX, n - at), out=du.ptr + 8 * at)

        def ph():
            eng.philox_random_dev([philox(5)], [n], out=du)
        row = verdict(alternate({"mt19937": lambda: timed(eng, mt)[:2], "philox": lambda: timed(eng, ph)[:2]}))
        check_head(du, 5)
        med = row["philox"]["device"]["median_ms"]
        row.update(n=n, segments=1, philox_gdraws_per_s=n / med / 1e6, philox_over_store_floor=med / (n * STORE_FLOOR_MS_PER_DRAW))
        res["generator"].append(row)
        print(show(f"(a) {n:>11} draws, one stream      ", row, ("mt19937", "philox")),
              f"mt/philox {row['ratio']:.2f} philox_wins {row['philox_wins']}; philox {row['philox_gdraws_per_s']:.1f} G draws/s,"
              f" {row['philox_over_store_floor']:.2f} x the store floor", flush=True)
        du.free()
    n = 10_000_000
    du = eng.alloc(8 * C * n)

    def mt_seeded():
        for c in range(C):
            np.random.seed(100 + c)
            eng.numpy_random_dev(n, out=du.ptr + 8 * c * n)

    def ph_seeded():
        eng.philox_random_dev([philox(100 + c) for c in range(C)], [n] * C, out=du, offsets=[c * n for c in range(C)])
    row = verdict(alternate({"mt19937": lambda: timed(eng, mt_seeded)[:2], "philox": lambda: timed(eng, ph_seeded)[:2]}))
    for c in (0, C - 1):
        check_head(du, 100 + c, c * n)
    med = row["philox"]["device"]["median_ms"]
    row.update(n=n, segments=C, philox_gdraws_per_s=C * n / med / 1e6, philox_over_store_floor=med / (C * n * STORE_FLOOR_MS_PER_DRAW))
    res["generator"].append(row)
    print(show(f"(a) {C} seeded stretches of {n} draws", row, ("mt19937", "philox")),
          f"mt/philox {row['ratio']:.2f} philox_wins {row['philox_wins']}; philox {row['philox_gdraws_per_s']:.1f} G draws/s,"
          f" {row['philox_over_store_floor']:.2f} x the store floor", flush=True)
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
    for n in LENGTHS:
        sizes = layer_sizes(n)
        g = torch.Generator(device="cuda").manual_seed(0)
        models = [{f"l{i:03d}": torch.randn(s, generator=g, device="cuda") * 0.05 + 0.001 * c for i, s in enumerate(sizes)} for c in range(C)]
        torch.cuda.synchronize()
        for b, compact in ((128, False), (20, True)):
            args = {"quantize": {"int_bits": b, "batch": False, "element_bits": 16, "padding": True, "secure": True}, "precompute": {"enable": False}}
            cohorts = {f: FlasheCohort(args, first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, compact=compact) for f in ("mt19937", "philox")}
            paths = {}

            def run(form):
                co = cohorts[form]
                co.set_iter_index(1)
                np.random.seed(11)
                rng = philox(11) if form == "philox" else None
                ms, wall, up = timed(co.cipher.engine, lambda: co.quantize_encrypt([W(dict(m)) for m in models], rng=rng))
                paths[form] = up.path
                return ms, wall
            row = alternate({f: (lambda f=f: run(f)) for f in cohorts})
            da, db = row["mt19937"]["device"], row["philox"]["device"]
            row["ratio"] = da["median_ms"] / db["median_ms"]
            row["spread_ms"] = max(da["range_ms"], db["range_ms"])
            row["philox_gain_outside_spread"] = bool(da["median_ms"] - db["median_ms"] > row["spread_ms"])
            row.update(n=n, int_bits=b, compact=compact, paths=paths)
            res["cohort_step"].append(row)
            print(show(f"(b) n {n:>9} int_bits {b}{' compact' if compact else ''} ({paths['philox']})", row, ("mt19937", "philox")),
                  f"rng=None / rng=Philox {row['ratio']:.2f}, outside the spread: {row['philox_gain_outside_spread']}", flush=True)
            del cohorts
            torch.cuda.empty_cache()
        del models


def main():
    res = {"alternations": ALTS, "library_sha256_16": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16], "generator": [],
           "cohort_step": []}
    print(f"{ALTS} alternations per form, device events (wall: host clock around the call and the wait for its last event)")
    if "b" in PART:
        import torch                  # (before the first engine: the framework then still finds its device)
        torch.zeros(1, device="cuda")
        torch.cuda.synchronize()
    if "a" in PART:
        part_a(Engine(KEY, 128, device=0), res)
    if "b" in PART:
        part_b(res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
