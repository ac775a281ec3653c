#!/usr/bin/env python3
"""The client-side round of a cohort of ten co-located clients on the 29.2 M-parameter, 57-layer model of client_step_tensors.py, held as
float32 or bfloat16 torch tensors on the GPU, b = 128: quantise + encrypt of all clients, their sum, decrypt + unquantise into out=.
Three forms, alternated inside one process after a warm-up, wall time around synchronised sections:
  (a) clients       ten FlasheClient.quantize_encrypt tensor steps, aggregate, one decrypt_unquantize(out=) -- what a caller ran before
                    FlasheCohort (22 AES streams per element position, a ten-operand reduce);
  (b) staged-chain  FlasheCohort with the fused launch switched off: a quantise pass per client, then the existing summed chain;
  (c) cohort-chain  FlasheCohort: one chained launch from the floats (11 streams), then one memory-bound pass.
Beside them the floor of (c)'s first launch: the existing summed chain alone (flashe_encrypt_batch_sum_dev) on pre-quantised one-limb
integer plaintexts of the same size, timed with device events.
Every block of REPS alternations gives one median per form; BLOCKS blocks give the box's spread (min - max of those medians).
LEG=c runs form (c) alone (for a kernel trace).  Prints one line per dtype and a final JSON line."""
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from flashe_amd import _lib, cipher as cm  # noqa: E402
from flashe_amd.block import FlasheClient, FlasheCohort  # noqa: E402


class W:
    def __init__(self, layers):
        self.walking_order = sorted(layers)
        self._weights = dict(layers)


cm.N_JOBS = 16
C = int(os.environ.get("CLIENTS", "10"))
sizes = [9408] + [s for s in (4096, 16384, 36864, 65536, 147456, 262144, 589824, 1048576, 2359296) for _ in range(6)] + [2048000, 1000]
args = {"quantize": {"int_bits": 128, "batch": False, "element_bits": 16, "padding": True, "secure": True}, "precompute": {"enable": False}}
REPS = int(os.environ.get("REPS", "5"))
BLOCKS = int(os.environ.get("BLOCKS", "3"))
LEG = os.environ.get("LEG", "")
KEY = bytes(range(32))


def round_clients(clients, models, out):
    cts = []
    for cl, m in zip(clients, models):
        w = cl.quantize_encrypt(W(dict(m)), device=True, normalize=True)
        cts.append(w._weights[w.walking_order[0]])
    agg = clients[0].cipher.aggregate(cts)
    clients[0].set_idx_list(list(range(C)))
    clients[0].decrypt_unquantize(W({sorted(models[0])[0]: agg}), out=out, unnormalize=True)


def round_cohort(co, models, out):
    up = co.quantize_encrypt([W(dict(m)) for m in models], normalize=True)
    co.decrypt_unquantize(out=out, unnormalize=True)
    return up.path


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), r


def floor_ms(eng, n):
    """The summed chain alone on integer plaintexts: median of REPS launches by device events."""
    g = torch.Generator(device="cuda").manual_seed(1)
    pts = [torch.randint(0, 2 ** 16, (n,), generator=g, device="cuda", dtype=torch.int64) for _ in range(C)]
    cts = [eng.alloc_vec(n) for _ in range(C)]
    sm = eng.alloc_vec(n)
    torch.cuda.synchronize()
    e0, e1 = eng.event(), eng.event()
    ms = []
    for i in range(REPS + 1):
        eng.record(e0)
        eng.encrypt_batch_sum_dev(1, list(range(C)), 1, n, cm.N_JOBS, [p.data_ptr() for p in pts], 1, cts, sm)
        eng.record(e1)
        ms.append(eng.elapsed_ms(e0, e1))
    return float(np.median(ms[1:]))


def main():
    n = sum(sizes)
    res = {"clients": C, "n": n, "reps": REPS, "blocks": BLOCKS, "library_sha256_16": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]}
    print(f"model: {len(sizes)} layers, {n / 1e6:.1f} M parameters, {C} clients; b = 128, element_bits = 16; {BLOCKS} blocks of {REPS} alternations")
    for dt in (torch.float32, torch.bfloat16):
        g = torch.Generator(device="cuda").manual_seed(0)
        models = [{f"l{i:03d}": (torch.randn(s, generator=g, device="cuda") * 0.05 + 0.001 * c).to(dt) for i, s in enumerate(sizes)} for c in range(C)]
        out = {k: torch.empty_like(t) for k, t in models[0].items()}
        clients = []
        for c in range(C):
            cl = FlasheClient(args)
            cl.create_cipher(c, C, KEY)
            cl.set_iter_index(1)
            clients.append(cl)
        cohorts = {}
        for form, prefer in (("b", "staged-chain"), ("c", None)):
            co = FlasheCohort(args, first_idx=0, n_local=C, num_clients=C, prp_seed=KEY)
            co.set_iter_index(1)
            co.prefer = prefer
            cohorts[form] = co
        forms = {"a": lambda: round_clients(clients, models, out), "b": lambda: round_cohort(cohorts["b"], models, out),
                 "c": lambda: round_cohort(cohorts["c"], models, out)}
        if LEG:
            forms = {LEG: forms[LEG]}
        np.random.seed(0)
        paths = {}
        for f, fn in forms.items():                            # warm-up of every form
            _ms, paths[f] = timed(fn)
        assert paths.get("b", "staged-chain") == "staged-chain" and paths.get("c", "cohort-chain") == "cohort-chain", paths
        medians = {f: [] for f in forms}
        for _b in range(BLOCKS):
            ms = {f: [] for f in forms}
            for _r in range(REPS):
                for f, fn in forms.items():
                    ms[f].append(timed(fn)[0])
            for f in forms:
                medians[f].append(float(np.median(ms[f])))
        name = str(dt).replace("torch.", "")
        row = {f: {"median_ms": float(np.median(v)), "min_ms": min(v), "max_ms": max(v)} for f, v in medians.items()}
        if not LEG:
            row["floor_ms"] = floor_ms(cohorts["c"].cipher.engine, n)
        res[name] = row
        print(name, " ".join(f"({f}) {r['median_ms']:8.2f} ms [{r['min_ms']:.2f} - {r['max_ms']:.2f}]" for f, r in row.items() if isinstance(r, dict)),
              f"floor {row.get('floor_ms', float('nan')):.3f} ms")
        del models, out, clients, cohorts, forms
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
