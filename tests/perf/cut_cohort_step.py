#!/usr/bin/env python3
"""The client step of a SHORT cohort -- many clients with a small model -- in three forms alternated inside ONE process after a warm-up:
  cut      FlasheCohort(cut=True) -> "cut-chain": the summed chain cut into runs of clients + one combine pass (two launches);
  staged   the same build with prefer="staged-chain": a quantise launch per client into plaintexts, then the summed batch encrypt;
  parent   the staged form of ANOTHER build of the library (the parent commit's, PARENT_LIB = its file name in flashe_amd/): the baseline.
Two levels:
  launches  the launches that differ, on draws that are already there, timed with device events on the engine's stream (table uploads
            included);
  step      wall time around the whole FlasheCohort.quantize_encrypt (+ sync): draws, tables, allocations, launches.
Per form the median of BLOCKS blocks of REPS runs, with the min - max of the block medians as the spread; `cut` wins a level over `parent`
when parent / cut - 1 exceeds the larger relative spread of the two.  The sums and the first and last ciphertext of cut and staged are
compared inside the run.  Shapes: 61,706 x 100 at b = 128 and compact b = 23; 1e6 x 10 and 1e6 x 50 at compact b = 20; 2e6 x 10 at b = 128.
SWEEP=1 (needs libflashe_hip_tuning.so): the cut launch at 61,706 x 100 forced to parts in {1, 2, 4, 8, 12, 16} through the tuning
library's FLASHE_CHAIN_PARTS knob, against the rule's own choice.  Prints one line per case and level and a final JSON line."""
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
from flashe_amd.block import FlasheCohort  # noqa: E402
from flashe_amd.engine import DeviceVector, Engine  # noqa: E402

KEY = bytes(range(32))
BLOCKS, REPS = int(os.environ.get("BLOCKS", "3")), int(os.environ.get("REPS", "5"))
PARENT_LIB = os.environ.get("PARENT_LIB", "")
SHAPES = [(61706, 100, 128, False), (61706, 100, 23, True), (1000000, 10, 20, True), (1000000, 50, 20, True), (2000000, 10, 128, False)]
NEW_SYMBOLS = ("flashe_cohort_cut_parts", "flashe_quantize_encrypt_cohort_cut_dev", "flashe_quantize_encrypt_cohort_cut_u32_dev")
cm.N_JOBS = 16


class W:
    def __init__(self, layers):
        self.walking_order = sorted(layers)
        self._weights = dict(layers)


class library:
    """`with library(name):` -- engines created inside bind that build of the library (an engine keeps the library it was created with)."""

    def __init__(self, name, old_abi=False):
        self.name, self.old_abi = name, old_abi

    def __enter__(self):
        self.saved = (_lib._lib, _lib.LIB_PATH, dict(_lib._SIGNATURES))
        _lib._lib, _lib.LIB_PATH = None, os.path.join(ROOT, "flashe_amd", self.name)
        if self.old_abi:                                       # (the parent build has no cut entry points)
            for s in NEW_SYMBOLS:
                _lib._SIGNATURES.pop(s, None)
        _lib.load()

    def __exit__(self, *exc):
        _lib._lib, _lib.LIB_PATH = self.saved[0], self.saved[1]
        _lib._SIGNATURES.clear()
        _lib._SIGNATURES.update(self.saved[2])


def args(b, eb):
    return {"quantize": {"int_bits": b, "batch": False, "element_bits": eb, "padding": True, "secure": True}, "precompute": {"enable": False}}


def layer_sizes(n, k=8):
    w = [(i % 7 + 1) ** 3 for i in range(k)]
    sizes = [n * x // (2 * sum(w)) for x in w]
    return sizes + [n - sum(sizes)]


def blocks_of(fn):
    meds = [float(np.median([fn() for _r in range(REPS)])) for _b in range(BLOCKS)]
    med = float(np.median(meds))
    return {"median_ms": med, "min_ms": min(meds), "max_ms": max(meds), "spread": (max(meds) - min(meds)) / med}


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


def verdict(row, base="parent"):
    if base not in row:
        base = "staged"
    row["baseline"] = base
    row["base_over_cut"] = row[base]["median_ms"] / row["cut"]["median_ms"]
    row["spread"] = max(row[base]["spread"], row["cut"]["spread"])
    row["cut_wins"] = bool(row["base_over_cut"] - 1.0 > row["spread"])
    row["cut_loses"] = bool(1.0 / row["base_over_cut"] - 1.0 > row["spread"])
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


def launch_forms(eng, b, eb, compact, models, sizes, C, with_cut):
    """{form: callable} of the launches that differ on one engine, plus the buffers they write."""
    n = sum(sizes)
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
    elem = 4 if compact else 16
    idxs = list(range(C))
    out = {}
    pts = [eng.alloc_vec(n) for _ in range(C)]
    s_cts, s_sum = [eng.alloc(elem * n) for _ in range(C)], eng.alloc(elem * n)

    def staged():
        for c in range(C):
            eng.quantize_batch_tensors_dev(tables[c], n, eb, b, du.ptr + 8 * c * n, n, pts[c])
        if compact:
            # (as FlasheCohort._launch_staged: the one-limb plaintexts are narrowed, then the compact summed encrypt)
            p32 = [DeviceVector(eng, n, 1, buf=pt).narrowed().buf for pt in pts]
            eng.encrypt_batch_sum_u32_dev(1, idxs, 1, n, cm.N_JOBS, p32, s_cts, s_sum)
        else:
            eng.encrypt_batch_sum_dev(1, idxs, 1, n, cm.N_JOBS, pts, eng.limbs, s_cts, s_sum)
    out["staged"] = (staged, (s_cts, s_sum, elem))
    if with_cut:
        parts = eng.cohort_cut_parts(C, n, cm.N_JOBS, compact=compact)
        assert parts, "the cut launch declines the shape"
        c_cts, c_sum, c_mask = [eng.alloc(elem * n) for _ in range(C)], eng.alloc(elem * n), eng.alloc(elem * n)
        scratch = eng.alloc((16 if n <= 100000 else parts) * n * elem * 2)       # (the short shapes: room for 16 pieces, the sweep)

        def cut():
            if compact:
                ok = eng.quantize_encrypt_cohort_cut_u32_dev(1, 0, n, cm.N_JOBS, rows, srcs, dts, eb, du, c_cts, c_sum, scratch)
            else:
                ok = eng.quantize_encrypt_cohort_cut_dev(1, 0, n, cm.N_JOBS, rows, srcs, dts, eb, du, c_cts, c_sum, c_mask, scratch)
            assert ok, "the cut launch declined the shape"
        out["cut"] = (cut, (c_cts, c_sum, elem))
        out["parts"] = parts
    out["keep"] = (du, pts)
    return out


def values(buf, n, elem):
    if elem == 4:
        return buf.download(np.uint32, n).astype(np.uint64)
    return buf.download(np.uint64, n * elem // 8).copy()


def launch_level(b, eb, compact, models, sizes, C):
    n = sum(sizes)
    eng = Engine(KEY, b, device=0)
    here = launch_forms(eng, b, eb, compact, models, sizes, C, True)
    forms = {"cut": lambda: timed(eng, here["cut"][0]), "staged": lambda: timed(eng, here["staged"][0])}
    if PARENT_LIB:
        with library(PARENT_LIB, old_abi=True):
            peng = Engine(KEY, b, device=0)
        there = launch_forms(peng, b, eb, compact, models, sizes, C, False)
        forms["parent"] = lambda: timed(peng, there["staged"][0])
    row = alternate(forms)
    # parity of cut against staged: the sum, the first and the last ciphertext
    (ccts, csum, ce), (scts, ssum, se) = here["cut"][1], here["staged"][1]
    eng.sync()
    for a, s in ((csum, ssum), (ccts[0], scts[0]), (ccts[-1], scts[-1])):
        assert np.array_equal(values(a, n, ce), values(s, n, se)), "the cut launch differs from the staged form"
    row["parts"] = here["parts"]
    return row


def step_level(b, eb, compact, models, C):
    cohorts = {}

    def make(prefer, cut):
        co = FlasheCohort(args(b, eb), first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, compact=compact, cut=cut)
        co.set_iter_index(1)
        co.prefer = prefer
        return co
    cohorts["cut"] = (make(None, True), "cut-chain")
    cohorts["staged"] = (make("staged-chain", True), "staged-chain")
    if PARENT_LIB:
        with library(PARENT_LIB, old_abi=True):
            cohorts["parent"] = (make(None, False), "staged-chain")

    def run(form):
        co, path = cohorts[form]
        eng = co.cipher.engine
        eng.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        up = co.quantize_encrypt([W(dict(m)) for m in models])
        eng.sync()
        ms = 1e3 * (time.perf_counter() - t0)
        assert up.path == path, (form, up.path)
        return ms
    return alternate({f: (lambda f=f: run(f)) for f in cohorts})


def sweep(models, sizes, C):
    """The cut launch at 61,706 x 100 with the piece count forced through the tuning library's knob."""
    os.environ["FLASHE_CHAIN_TUNE"] = "1"
    out = []
    with library("libflashe_hip_tuning.so"):
        for b, eb, compact in ((128, 16, False), (23, 16, True)):
            eng = Engine(KEY, b, device=0)
            os.environ.pop("FLASHE_CHAIN_PARTS", None)
            forms = launch_forms(eng, b, eb, compact, models, sizes, C, True)
            rule = forms["parts"]
            row = {"int_bits": b, "compact": compact, "rule_parts": rule, "parts": {}}
            for k in (0, 1, 2, 4, 8, 12, 16):

                def run(k=k):
                    if k:
                        os.environ["FLASHE_CHAIN_PARTS"] = str(k)
                    else:
                        os.environ.pop("FLASHE_CHAIN_PARTS", None)
                    return timed(eng, forms["cut"][0])
                run()
                run()
                row["parts"]["rule" if not k else str(k)] = blocks_of(run)
            os.environ.pop("FLASHE_CHAIN_PARTS", None)
            print(f"sweep int_bits {b} rule = {rule} parts:", " ".join(f"{k} {v['median_ms']:.4f} [{v['min_ms']:.4f} - {v['max_ms']:.4f}]" for k, v in row["parts"].items()),
                  flush=True)
            out.append(row)
    os.environ.pop("FLASHE_CHAIN_TUNE", None)
    return out


def main():
    res = {"blocks": BLOCKS, "reps": REPS, "parent": PARENT_LIB, "library_sha256_16": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16],
           "cases": []}
    print(f"n_jobs {cm.N_JOBS}; median of {BLOCKS} blocks of {REPS}, [min - max of the block medians]; baseline {'parent ' + PARENT_LIB if PARENT_LIB else 'staged'}")
    for n, C, b, compact in SHAPES:
        eb = min(16, b - (C - 1).bit_length())
        sizes = layer_sizes(n)
        g = torch.Generator(device="cuda").manual_seed(0)
        models = [{f"l{i:03d}": torch.randn(s, generator=g, device="cuda") * 0.05 + 0.001 * c for i, s in enumerate(sizes)} for c in range(C)]
        torch.cuda.synchronize()
        case = {"n": n, "clients": C, "int_bits": b, "compact": compact, "element_bits": eb}
        for name, fn in (("launches", lambda: launch_level(b, eb, compact, models, sizes, C)), ("step", lambda: step_level(b, eb, compact, models, C))):
            row = verdict(fn())
            case[name] = row
            print(f"n {n:>8} x {C:>3} int_bits {b:>3}{' compact' if compact else '':<8} {name:<8}",
                  " ".join(f"{f} {r['median_ms']:8.3f} ms [{r['min_ms']:.3f} - {r['max_ms']:.3f}]" for f, r in row.items() if isinstance(r, dict)),
                  f"{row['baseline']}/cut {row['base_over_cut']:.3f} spread {100 * row['spread']:.1f} % cut_wins {row['cut_wins']} cut_loses {row['cut_loses']}"
                  + (f" parts {row['parts']}" if "parts" in row else ""), flush=True)
        res["cases"].append(case)
        if os.environ.get("SWEEP") == "1" and (n, C, b) == (61706, 100, 128):
            res["sweep"] = sweep(models, sizes, C)
        del models
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
