#!/usr/bin/env python3
"""The front end of a sparse cohort's uploads -- from the first quantise launch to the last ciphertext store; the draws and the aggregate
are outside -- at the widths the shipped sparse jobs run (int_bits 20 and 23, element_bits 16), float32 compact layers in HBM: ten
clients x K = 2,920,000 and fifty clients x K = 255,570.  Three forms, alternated inside ONE process after a warm-up, timed with device
events on each engine's stream:
  fused    Engine.quantize_encrypt_sparse_cohort_dev: one chained launch from the floats (20 bytes moved per value and client);
  staged   Engine.quantize_cohort_dev into one-limb plaintexts, then ONE batched single-mask encrypt (Engine.encrypt_batch_dev: what
           flashe_sparse_encrypt_aggregate_dev's two-call branch runs for clients of one k) -- 36 bytes;
  parent   the staged form as the parent commit ran it: quantize_cohort_dev, then one Engine.encrypt_dev per client, on a build of the
           parent commit's library (PARENT_LIB, a file name in flashe_amd/; loaded as tests/perf/ab_compact_libs.py loads its builds).
           Left out when that file is missing.
The forms' uploads and quantised zeros are compared byte for byte inside the run.  A timed window holds CALLS calls of one form (ms per
call is reported); ALTS alternations (at least nine) give a median per form; `spread` is (max - min) / median of a form's own alternations, and the fused form `wins` over another one when other / fused - 1
exceeds the larger of the two spreads.  LEG=fused (staged, parent) runs one form alone (for a kernel trace).  Prints one line per case
and a final JSON line."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flashe_amd import _lib  # noqa: E402
from flashe_amd.engine import SCHEME_SINGLE, Engine  # noqa: E402

KEY = bytes(range(32))
EB, J, IT = 16, 16, 1
ALTS = max(9, int(os.environ.get("ALTS", "9")))
CALLS = max(1, int(os.environ.get("CALLS", "5")))          # calls of a form inside one timed window
LEG = os.environ.get("LEG", "")
PARENT_LIB = os.environ.get("PARENT_LIB", "libflashe_hip_parent.so")
SHAPES = [tuple(int(x) for x in s.split("x")) for s in os.environ.get("SHAPES", "10x2920000,50x255570").split(",")]      # clients x K
WIDTHS = [int(v) for v in os.environ.get("WIDTHS", "20,23").split(",")]
PRODUCT_LIB = os.path.basename(_lib.LIB_PATH)


NEW_SYMBOLS = ("flashe_quantize_encrypt_sparse_cohort_dev",)       # what the parent build does not export


def engine_from(name, b):
    _lib._lib = None
    _lib.LIB_PATH = os.path.join(ROOT, "flashe_amd", name)
    absent = {k: _lib._SIGNATURES.pop(k) for k in NEW_SYMBOLS} if name == PARENT_LIB else {}
    try:
        return Engine(KEY, b)
    finally:
        _lib._SIGNATURES.update(absent)


def layer_sizes(n, k=40):
    w = [(i % 7 + 1) ** 3 for i in range(k)]
    sizes = [max(1, n * x // (2 * sum(w))) for x in w]
    return sizes + [n - sum(sizes)]


def timed(eng, fn):
    e0, e1 = eng.event(), eng.event()
    eng.sync()
    eng.record(e0)
    for _r in range(CALLS):
        fn()
    eng.record(e1)
    eng.sync()
    ms = eng.elapsed_ms(e0, e1) / CALLS
    eng.event_destroy(e0)
    eng.event_destroy(e1)
    return ms


def stats(ms):
    med = float(np.median(ms))
    return {"median_ms": med, "min_ms": float(min(ms)), "max_ms": float(max(ms)), "spread": float((max(ms) - min(ms)) / med)}


class Side:
    """One engine with the cohort's sources, draws and outputs on it."""

    def __init__(self, lib, b, C, K, sizes):
        self.eng, self.C, self.K = engine_from(lib, b), C, K
        eng = self.eng
        starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
        alphas = [0.2 + 0.01 * (i % 5) for i in range(len(sizes))]
        self.rows = [(int(starts[i]), None, alphas[i], 0.0, _lib.TENSOR_F32, 0) for i in range(len(sizes))]
        g = np.random.Generator(np.random.PCG64(7))
        self.keep, self.srcs = [], []
        for c in range(C):
            x = (g.standard_normal(K) * 0.1 + 0.001 * c).astype(np.float32)
            d = eng.upload(x)
            self.keep.append(d)
            self.srcs.append([d.ptr + 4 * int(s) for s in starts])
        self.dts = [[_lib.TENSOR_F32] * len(sizes) for _ in range(C)]
        self.du = eng.alloc(8 * C * (K + 1))
        np.random.seed(3)
        for at in range(0, C * (K + 1), 1 << 26):
            eng.numpy_random_dev(min(1 << 26, C * (K + 1) - at), out=self.du.ptr + 8 * at)
        self.zzz = [0.0] * C
        self.idx = list(range(C))
        self.pts = [eng.alloc_vec(K, 1) for _ in range(C)]
        self.ups = [eng.alloc_vec(K + 1, 1) for _ in range(C)]
        self.zeros = eng.alloc(8 * C + 16)

    def _quantise(self):
        self.eng.quantize_cohort_dev(self.K, self.rows, self.srcs, self.dts, EB, self.du, self.K + 1, self.zzz, True, self.pts,
                                     [u.ptr + 8 * self.K for u in self.ups], self.zeros)

    def fused(self):
        assert self.eng.quantize_encrypt_sparse_cohort_dev(IT, self.idx, self.K, J, self.rows, self.srcs, self.dts, EB, self.du, self.K + 1, self.zzz, True,
                                                           self.ups, self.zeros), "the chained launch declined the shape"

    def staged(self):
        self._quantise()
        self.eng.encrypt_batch_dev(IT, self.idx, SCHEME_SINGLE, self.K, J, self.pts, 1, self.ups)

    def parent(self):
        self._quantise()
        for c in range(self.C):
            self.eng.encrypt_dev(IT, self.idx[c], SCHEME_SINGLE, self.K, J, self.pts[c], 1, self.ups[c])

    def digest(self):
        h = hashlib.sha256()
        for u in self.ups:
            h.update(u.download(np.uint64, self.K + 1).tobytes())
        h.update(self.zeros.download(np.uint64, self.C).tobytes())
        return h.hexdigest()

    def clear(self):
        for u in self.ups:
            self.eng.memset_dev(u, 0, 8 * (self.K + 1))
        self.eng.memset_dev(self.zeros, 0, 8 * self.C)
        self.eng.sync()


def main():
    have_parent = os.path.exists(os.path.join(ROOT, "flashe_amd", PARENT_LIB))
    sha = lambda name: hashlib.sha256(open(os.path.join(ROOT, "flashe_amd", name), "rb").read()).hexdigest()[:16]      # noqa: E731
    res = {"alternations": ALTS, "calls_per_window": CALLS, "library_sha256_16": sha(PRODUCT_LIB), "parent_library_sha256_16": sha(PARENT_LIB) if have_parent else None, "cases": []}
    print(f"element_bits {EB}, n_jobs {J}; {ALTS} alternations per form of {CALLS} calls each, device events, ms per call; parent build: {PARENT_LIB if have_parent else 'absent'}", flush=True)
    for C, K in SHAPES:
        sizes = layer_sizes(K)
        for b in WIDTHS:
            here = Side(PRODUCT_LIB, b, C, K, sizes)
            forms = {"fused": here.fused, "staged": here.staged}
            sides = {"fused": here, "staged": here}
            if have_parent:
                there = Side(PARENT_LIB, b, C, K, sizes)
                forms["parent"], sides["parent"] = there.parent, there
            if LEG:
                forms = {LEG: forms[LEG]}
            digests = {}
            for f, fn in forms.items():                                            # warm-up of every form, and the parity of what it wrote
                sides[f].clear()
                fn()
                sides[f].eng.sync()
                digests[f] = sides[f].digest()
            assert len(set(digests.values())) == 1, ("the forms' uploads differ", digests)
            ms = {f: [] for f in forms}
            for _a in range(ALTS):
                for f, fn in forms.items():
                    ms[f].append(timed(sides[f].eng, fn))
            row = {f: stats(v) for f, v in ms.items()}
            case = {"clients": C, "K": K, "int_bits": b, "forms_identical": True, **row}
            line = " ".join(f"{f} {r['median_ms']:8.3f} ms [{r['min_ms']:.3f} - {r['max_ms']:.3f}]" for f, r in row.items())
            if "fused" in row:
                for other in ("staged", "parent"):
                    if other in row:
                        ratio = row[other]["median_ms"] / row["fused"]["median_ms"]
                        spread = max(row[other]["spread"], row["fused"]["spread"])
                        case[f"{other}_over_fused"], case[f"fused_wins_over_{other}"] = ratio, bool(ratio - 1.0 > spread)
                        line += f" | {other}/fused {ratio:.3f} spread {100 * spread:.1f} % wins {case[f'fused_wins_over_{other}']}"
            print(f"clients {C:>3} K {K:>8} int_bits {b}: {line}", flush=True)
            res["cases"].append(case)
            del here, sides, forms
    print(json.dumps(res))


if __name__ == "__main__":
    main()
