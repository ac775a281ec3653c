#!/usr/bin/env python3
"""In-process A/B of the sparse single-mask passes at int_bits <= 64: the passes with the PRF inside (span_prf_small_kernel: one launch
per group of 64 clients for the encrypt + aggregate and for the decrypt) against the two-call forms they replace -- one encrypt per client
(or one batched encrypt) and the sorted span reduce of what they wrote; the stream + scatter per client and a combine for the decrypt
(what flashe_sparse_decrypt_dev runs on unsorted lists, and ran on sorted ones before).  Forms alternate call by call; parity of every
output between the forms is checked inside the run.

usage: ab_sparse_small.py [reps]      shapes: config 5's (25.6 M positions, 50 clients, 1 % each) at b = 20 and 64, the sparse jobs'
10 % density at b = 20 (10 clients)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from flashe_amd.engine import SCHEME_SINGLE, Engine  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
CALLS = 5
TOTAL, J = 25_600_000, 16


def lists(total, C, k, seed):
    out = []
    for c in range(C):
        r = np.random.Generator(np.random.PCG64(seed + c))
        out.append(np.sort(r.choice(total, k, replace=False)).astype(np.uint32))
    return out


def timed(eng, evs, fn):
    eng.record(evs[0])
    for _ in range(CALLS):
        fn()
    eng.record(evs[1])
    eng.sync()
    return eng.elapsed_ms(evs[0], evs[1]) / CALLS


def shape(b, C, density, seed):
    eng = Engine(bytes(range(32)), b, device=0)
    k = int(TOTAL * density)
    locs = lists(TOTAL, C, k, seed)
    ks = [k] * C
    rng = np.random.Generator(np.random.PCG64(seed + 999))
    pts = [rng.integers(0, 2 ** b, k, dtype=np.uint64) for _ in range(C)]
    idx = list(range(C))
    zeros = [(1 << (b - 1)) + c for c in range(C)]
    dl, dp = [eng.upload(l) for l in locs], [eng.upload(p) for p in pts]
    del pts
    ct_a, ct_b = [eng.alloc_vec(k) for _ in range(C)], [eng.alloc_vec(k) for _ in range(C)]
    agg_a, agg_b, dec_a, dec_b = (eng.alloc_vec(TOTAL) for _ in range(4))
    bnd = eng.span_bounds(TOTAL, dl, ks)
    forms = {
        # (the whole-vector call keeps the two calls at int_bits <= 64 -- DESIGN.md 4.3 -- so the fused encrypting pass is timed as one
        # position range over the whole vector)
        "enc_whole_call": lambda: eng.sparse_encrypt_aggregate_dev(3, idx, dl, ks, dp, 1, zeros, TOTAL, J, ct_a, agg_a),
        "enc_fused_bounds": lambda: eng.sparse_encrypt_aggregate_dev(3, idx, dl, ks, dp, 1, zeros, TOTAL, J, ct_a, agg_a, bounds=bnd,
                                                                     position_range=(0, TOTAL)),      # (last to write ct_a / agg_a: their parity)
        "enc_two_call": lambda: ([eng.encrypt_dev(3, idx[c], SCHEME_SINGLE, k, J, dp[c], 1, ct_b[c]) for c in range(C)],
                                 eng.sparse_aggregate_dev(TOTAL, dl, ks, ct_b, zeros, agg_b, sorted_lists=True)),
        "enc_batch_two_call": lambda: (eng.encrypt_batch_dev(3, idx, SCHEME_SINGLE, k, J, dp, 1, ct_b),
                                       eng.sparse_aggregate_dev(TOTAL, dl, ks, ct_b, zeros, agg_b, sorted_lists=True)),
        "dec_fused": lambda: eng.sparse_decrypt_dev(3, dl, ks, TOTAL, J, agg_a, dec_a, sorted_lists=True),
        "dec_fused_bounds": lambda: eng.sparse_decrypt_dev(3, dl, ks, TOTAL, J, agg_a, dec_a, bounds=bnd),
        "dec_two_call": lambda: eng.sparse_decrypt_dev(3, dl, ks, TOTAL, J, agg_a, dec_b, sorted_lists=False),
    }
    evs = [eng.event() for _ in range(2)]
    for f in forms.values():                     # warm-up (and the allocations of the ctx's scratch)
        f()
    eng.sync()
    times = {n: [] for n in forms}
    for _ in range(REPS):
        for n, f in forms.items():
            times[n].append(timed(eng, evs, f))
    # parity between the forms
    for c in range(C):
        assert np.array_equal(ct_a[c].download(np.uint64, k), ct_b[c].download(np.uint64, k)), (b, c, "ciphertext")
    assert np.array_equal(agg_a.download(np.uint64, TOTAL), agg_b.download(np.uint64, TOTAL)), (b, "aggregate")
    assert np.array_equal(dec_a.download(np.uint64, TOTAL), dec_b.download(np.uint64, TOTAL)), (b, "decrypt")
    res = {"b": b, "total": TOTAL, "C": C, "k": k, "n_jobs": J, "reps": REPS, "calls_per_rep": CALLS, "parity": "ok",
           "ms_median": {n: float(np.median(v)) for n, v in times.items()}, "ms_min": {n: float(np.min(v)) for n, v in times.items()},
           "ms_max": {n: float(np.max(v)) for n, v in times.items()}}
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    for b, C, dens, seed in [(20, 50, 0.01, 3000), (64, 50, 0.01, 3000), (20, 10, 0.10, 4000)]:
        shape(b, C, dens, seed)
