#!/usr/bin/env python3
"""A client's step from a training framework's tensors: the ResNet-50-sized model of tests/perf/client_step.py (29.2 M parameters as 57
layers) held as float32 or bfloat16 torch tensors on the GPU.  Both sides of the step -- normalize + quantise + encrypt, and decrypt +
unquantise + unnormalize back into the model's parameters -- timed two ways on one box:
  host path   the caller copies every layer to the host (t.float().cpu().numpy()), FlasheClient.quantize_encrypt(normalize=True) uploads it,
              decrypt_unquantize(unnormalize=True) returns float64 host arrays, the caller copies them back into its parameters;
  tensors     quantize_encrypt(tensors, normalize=True) reads the layers in place, decrypt_unquantize(out=params, unnormalize=True) writes
              them in place; no layer byte crosses PCIe.
The decrypt side decrypts the client's own ciphertext (one client), which costs what the aggregate's decrypt costs."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from flashe_amd import cipher as cm  # noqa: E402
from flashe_amd.block import FlasheClient  # noqa: E402


class W:
    def __init__(self, layers):
        self.walking_order = sorted(layers)
        self._weights = dict(layers)


cm.N_JOBS = 16
sizes = [9408] + [s for s in (4096, 16384, 36864, 65536, 147456, 262144, 589824, 1048576, 2359296) for _ in range(6)] + [2048000, 1000]
args = {"quantize": {"int_bits": 128, "batch": False, "element_bits": 16, "padding": True, "secure": True}, "precompute": {"enable": False}}
REPS = int(os.environ.get("REPS", "5"))


def client():
    cl = FlasheClient(args)
    cl.create_cipher(0, 1, bytes(range(32)))
    cl.set_iter_index(1)
    return cl


def step_host(cl, params):
    t0 = time.perf_counter()
    host = {k: p.float().cpu().numpy() for k, p in params.items()}
    w = cl.quantize_encrypt(W(host), device=True, normalize=True)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    cl.set_idx_list([0])
    res = cl.decrypt_unquantize(W({k: v for k, v in w._weights.items()}), unnormalize=True)
    for k, p in params.items():
        p.copy_(torch.from_numpy(np.ascontiguousarray(res._weights[k])).to(p.dtype))
    torch.cuda.synchronize()
    return t0, t1, time.perf_counter()


def step_tensors(cl, params):
    t0 = time.perf_counter()
    w = cl.quantize_encrypt(W(dict(params)), device=True, normalize=True)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    cl.set_idx_list([0])
    cl.decrypt_unquantize(W({k: v for k, v in w._weights.items()}), out=params, unnormalize=True)
    torch.cuda.synchronize()
    return t0, t1, time.perf_counter()


def main():
    print(f"model: {len(sizes)} layers, {sum(sizes) / 1e6:.1f} M parameters; b = 128, element_bits = 16; median of {REPS} steps after a warm-up")
    for dt in (torch.float32, torch.bfloat16):
        for name, fn in (("host path", step_host), ("tensors  ", step_tensors)):
            g = torch.Generator(device="cuda").manual_seed(0)
            params = {f"l{i:03d}": (torch.randn(s, generator=g, device="cuda") * 0.05).to(dt) for i, s in enumerate(sizes)}
            cl = client()
            np.random.seed(0)
            fn(cl, params)
            enc, dec = [], []
            for _ in range(REPS):
                t0, t1, t2 = fn(cl, params)
                enc.append(t1 - t0)
                dec.append(t2 - t1)
            e, d = 1e3 * float(np.median(enc)), 1e3 * float(np.median(dec))
            print(f"{str(dt).replace('torch.', ''):9s} {name}: encrypt side {e:7.2f} ms, decrypt side {d:7.2f} ms, step {e + d:7.2f} ms")


if __name__ == "__main__":
    main()
