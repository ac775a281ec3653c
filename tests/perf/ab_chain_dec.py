#!/usr/bin/env python3
"""The headline round -- ten 1e7-element encrypts as one chain, their sum and the decrypt of the sum, int_bits 128 -- under several BUILDS
of the library alternated inside one process and timed by events: a build that has flashe_encrypt_batch_sum_decrypt_dev runs the round
as that ONE call (prf_dec_sum128_kernel), a build from before it as flashe_encrypt_batch_sum_dev (prf_dmask_sum128_kernel) followed by
flashe_decrypt_dev (combine_wide_kernel).  Per build: the summed chain launch alone and the whole round, min / median / max over the
alternations; outputs compared byte for byte.
usage: ab_chain_dec.py <.so in flashe_amd/> <.so> [...]     (AB_REPS alternations, default 6; AB_N / AB_C: vector length and clients;
       FLASHE_CHAIN_DEC=0 makes a new build run the two calls as well)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flashe_amd import _lib  # noqa: E402
from flashe_amd.engine import SCHEME_DOUBLE, Engine  # noqa: E402

NEW = "flashe_encrypt_batch_sum_decrypt_dev"


def engine_from(name):
    """(engine, has the one-call round?) -- a build from before the entry point is bound without it"""
    _lib._lib = None
    _lib.LIB_PATH = os.path.join(ROOT, "flashe_amd", name)
    sig = _lib._SIGNATURES[NEW]
    try:
        return Engine(bytes(range(32)), 128), True
    except AttributeError:
        del _lib._SIGNATURES[NEW]
        try:
            _lib._lib = None
            return Engine(bytes(range(32)), 128), False
        finally:
            _lib._SIGNATURES[NEW] = sig


libs = sys.argv[1:]
n, C, J, K = int(os.environ.get("AB_N", "10000000")), int(os.environ.get("AB_C", "10")), 16, 10
reps = int(os.environ.get("AB_REPS", "6"))
st = {}
for name in libs:
    eng, one_call = engine_from(name)
    pts = [eng.upload(np.random.default_rng(c).integers(0, 2 ** 63, n, dtype=np.uint64)) for c in range(C)]
    cts = [eng.alloc_vec(n) for _ in range(C)]
    dsum, dec = eng.alloc_vec(n), eng.alloc_vec(n)
    st[name] = (eng, one_call, pts, cts, dsum, dec, [eng.event() for _ in range(2 * K + 1)])
idx = list(range(C))


def one_round(s, it, k=None):
    eng, one_call, pts, cts, dsum, dec, ev = s
    if one_call:
        eng.encrypt_batch_sum_decrypt_dev(it, idx, SCHEME_DOUBLE, n, J, pts, 1, cts, dsum, dec)
    else:
        eng.encrypt_batch_sum_dev(it, idx, SCHEME_DOUBLE, n, J, pts, 1, cts, dsum)
    if k is not None:
        eng.record(ev[2 * k + 1])
    if not one_call:
        eng.decrypt_dev(it, [C], [0], n, J, dsum, dec)
    if k is not None:
        eng.record(ev[2 * k + 2])


res = {name: [] for name in libs}
for rep in range(reps + 1):
    for name in libs:
        eng, ev = st[name][0], st[name][6]
        for it in range(3):
            one_round(st[name], it)
        eng.record(ev[0])
        for k in range(K):
            one_round(st[name], k, k)
        eng.sync()
        if rep:                                              # (the first alternation warms the clocks)
            res[name].append((np.mean([eng.elapsed_ms(ev[2 * k], ev[2 * k + 1]) for k in range(K)]),
                              np.mean([eng.elapsed_ms(ev[2 * k], ev[2 * k + 2]) for k in range(K)])))
ref = None
for name in libs:
    eng, one_call, pts, cts, dsum, dec, ev = st[name]
    got = tuple(b.download(np.uint64, 2 * n).tobytes() for b in (cts[3], dsum, dec))
    ref = ref or got
    a = np.array(res[name])
    fmt = lambda v: f"min {v.min():.4f} med {np.median(v):.4f} max {v.max():.4f}"          # noqa: E731
    print(f"{name:28s} {'one call ' if one_call else 'two calls'}  chain launch {fmt(a[:, 0])}   round {fmt(a[:, 1])} ms   "
          f"ct / sum / dec identical to the first build: {got == ref}", flush=True)
