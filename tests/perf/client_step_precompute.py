#!/usr/bin/env python3
"""The client step of precompute jobs, each direction timed on its own, with prepare_encrypt / prepare_decrypt timed apart:
  fused+cache   quantize_encrypt / decrypt_unquantize with the masks the ctx holds (no AES in the step)
  call by call  the same with fuse=False (the reference's sequence: host quantiser, object ints, cipher.encrypt / decrypt)
  fused online  the fused step without a cache (the PRF runs inside the codec launch)
Sizes: the flat lengths of the six shipped precompute configs (one layer of num_params values at b = 20; at b = 120 batched one layer of
6 x num_params values, which batches into num_params elements) and the 57-layer ResNet-50-sized list; host float32 layers and float32
torch tensors.  Every time ends in a device synchronise; median of REPS steps after a warm-up (call by call: CBC_REPS, skipped above
CBC_MAX values)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from flashe_amd import cipher as cm  # noqa: E402
from flashe_amd.block import FlasheClient  # noqa: E402

REPS = int(os.environ.get("REPS", "7"))
CBC_REPS = int(os.environ.get("CBC_REPS", "2"))
CBC_MAX = int(os.environ.get("CBC_MAX", "2000000"))
C = 10
RESNET = [9408] + [s for s in (4096, 16384, 36864, 65536, 147456, 262144, 589824, 1048576, 2359296) for _ in range(6)] + [2048000, 1000]


class W:
    def __init__(self, layers):
        self.walking_order = sorted(layers)
        self._weights = dict(layers)


def n_ct(sizes, b, batch):
    if not batch:
        return sum(sizes)
    bs = b // (16 + int(np.ceil(np.log2(C))))
    return sum((s + bs - 1) // bs for s in sizes)


def client(b, batch, sizes, precompute, fuse):
    args = {"quantize": {"int_bits": b, "batch": batch, "element_bits": 16, "padding": True, "secure": True},
            "precompute": {"enable": precompute, "num_params": n_ct(sizes, b, batch)}}
    cl = FlasheClient(args)
    cl.create_cipher(3, C, bytes(range(32)))
    cl.fuse = fuse
    cl.set_iter_index(1)
    return cl


def sync(cl):
    cl.cipher.engine.sync()
    torch.cuda.synchronize()


def one_step(cl, layers, tensors, precompute):
    """(prepare_encrypt, encrypt, prepare_decrypt, decrypt) seconds of one step."""
    t = []
    t0 = time.perf_counter()
    if precompute:
        cl.set_iter_index(0)
        cl.prepare_encrypt()
        cl.set_iter_index(1)
    sync(cl)
    t.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    w = cl.quantize_encrypt(W(dict(layers)), device=True)
    sync(cl)
    t.append(time.perf_counter() - t0)
    ct = w._weights[w.walking_order[0]]
    t0 = time.perf_counter()
    if precompute:
        cl.prepare_decrypt()
    sync(cl)
    t.append(time.perf_counter() - t0)
    cl.set_idx_list(list(range(C)))
    t0 = time.perf_counter()
    if tensors and cl.fuse:
        out = {k: torch.empty_like(v) for k, v in layers.items()}
        cl.decrypt_unquantize(W({w.walking_order[0]: ct}), out=out)
    else:
        cl.decrypt_unquantize(W({w.walking_order[0]: ct}))
    sync(cl)
    t.append(time.perf_counter() - t0)
    return t


def measure(name, sizes, b, batch):
    g = torch.Generator(device="cuda").manual_seed(0)
    dev = {f"l{i:03d}": torch.randn(s, generator=g, device="cuda", dtype=torch.float32) * 0.05 for i, s in enumerate(sizes)}
    host = {k: v.cpu().numpy() for k, v in dev.items()}
    total = sum(sizes)
    for src, layers in (("host", host), ("f32 tensors", dev)):
        for path, pre, fuse in (("fused+cache", True, True), ("call by call", True, False), ("fused online", False, True)):
            if not fuse and src != "host":
                continue                                         # (the call-by-call step takes host layers only)
            if not fuse and total > CBC_MAX:
                print(f"{name:30s} {src:11s} {path:12s}  (skipped: {total} values > CBC_MAX)", flush=True)
                continue
            lay = layers
            cl = client(b, batch, sizes, pre, fuse)
            np.random.seed(0)
            one_step(cl, lay, src != "host", pre)
            runs = [one_step(cl, lay, src != "host", pre) for _ in range(REPS if fuse else CBC_REPS)]
            med = [1e3 * float(np.median([r[i] for r in runs])) for i in range(4)]
            prep = f"prepare_encrypt {med[0]:8.3f} ms, prepare_decrypt {med[2]:8.3f} ms" if pre else " " * 50
            print(f"{name:30s} {src:11s} {path:12s}  encrypt {med[1]:9.3f} ms  decrypt {med[3]:9.3f} ms   {prep}", flush=True)


def main():
    cm.N_JOBS = 16
    print(f"C = {C} clients' masks, element_bits = 16, median of {REPS} (call by call: {CBC_REPS}) after a warm-up; one MI355X")
    for p in (1206590, 655187, 272474):
        measure(f"b=20  {p} values", [p], 20, False)
    for e in (201101, 109199, 45433):
        measure(f"b=120 batched {e} elements", [6 * e], 120, True)
    measure("b=20  ResNet-50 list (57 layers)", RESNET, 20, False)
    measure("b=120 batched ResNet-50 list", RESNET, 120, True)


if __name__ == "__main__":
    main()
