#!/usr/bin/env python3
"""The aggregator's degree scaling around a client's step (jzf_aggregator.py:676, :902-907) on the ResNet-50-sized model of
tests/perf/client_step_tensors.py: 29.2 M parameters as 57 float32 torch tensors on the GPU, b = 128, normalize / unnormalize on.  Both
sides of the step are timed with device events on the stream the client runs on, three forms alternated in one process:
  (a) framework   the only way without the arguments: a framework `mul` per layer in front of quantize_encrypt; behind it
                  decrypt_unquantize(out=float64 scratch, unnormalize=False), a framework division by total / degree, then unnormalize on
                  the host (its np.mean / np.std are the next round's statistics), `/ degree`, `+ last round` and the copy back;
  (b) arguments   quantize_encrypt(degree=), decrypt_unquantize(out=params, unnormalize=True, total_degree=, last_round=params);
  (c) no degree   the same step without any scaling.
The expectation to report against: (b) costs what (c) costs, plus the divisions.  The decrypt side decrypts the client's own upload."""
import os
import sys

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
REPS = max(7, int(os.environ.get("REPS", "7")))
DEGREE, TOTAL = 5000.0, 13700.0


def client():
    cl = FlasheClient(args, stream=torch.cuda.current_stream().cuda_stream)
    cl.create_cipher(0, 1, bytes(range(32)))
    cl.set_iter_index(1)
    return cl


def events():
    return [torch.cuda.Event(enable_timing=True) for _ in range(3)]


def step_framework(cl, params, ev):
    ev[0].record()
    scaled = {k: p * DEGREE for k, p in params.items()}
    w = cl.quantize_encrypt(W(scaled), device=True, normalize=True)
    ev[1].record()
    cl.set_idx_list([0])
    tmp = {k: torch.empty(p.shape, dtype=torch.float64, device="cuda") for k, p in params.items()}
    cl.decrypt_unquantize(W(dict(w._weights)), out=tmp, unnormalize=False)
    s = TOTAL / DEGREE
    host = cl.unnormalize(W({k: (t / s).cpu().numpy() for k, t in tmp.items()}))
    for k, p in params.items():
        p.copy_(torch.from_numpy(p.cpu().numpy() + host._weights[k] / DEGREE).to(p.dtype))
    ev[2].record()


def step_arguments(cl, params, ev):
    ev[0].record()
    w = cl.quantize_encrypt(W(dict(params)), device=True, normalize=True, degree=DEGREE)
    ev[1].record()
    cl.set_idx_list([0])
    cl.decrypt_unquantize(W(dict(w._weights)), out=params, unnormalize=True, total_degree=TOTAL, last_round=params)
    ev[2].record()


def step_plain(cl, params, ev):
    ev[0].record()
    w = cl.quantize_encrypt(W(dict(params)), device=True, normalize=True)
    ev[1].record()
    cl.set_idx_list([0])
    cl.decrypt_unquantize(W(dict(w._weights)), out=params, unnormalize=True)
    ev[2].record()


def main():
    forms = [("(a) framework", step_framework), ("(b) arguments", step_arguments), ("(c) no degree", step_plain)]
    print(f"model: {len(sizes)} float32 layers, {sum(sizes) / 1e6:.1f} M parameters; b = 128, element_bits = 16, normalize / unnormalize on; "
          f"degree {DEGREE:g} of {TOTAL:g}; {REPS} alternated steps per form after a warm-up, device events")
    state = {}
    for name, _fn in forms:
        g = torch.Generator(device="cuda").manual_seed(0)
        state[name] = (client(), {f"l{i:03d}": torch.randn(s, generator=g, device="cuda") * 0.05 for i, s in enumerate(sizes)})
    times = {name: ([], []) for name, _fn in forms}
    np.random.seed(0)
    for rep in range(REPS + 1):                                  # (the first round warms every form up and is dropped)
        for name, fn in forms:
            cl, params = state[name]
            ev = events()
            fn(cl, params, ev)
            torch.cuda.synchronize()
            if rep:
                times[name][0].append(ev[0].elapsed_time(ev[1]))
                times[name][1].append(ev[1].elapsed_time(ev[2]))
    for name, _fn in forms:
        enc, dec = np.array(times[name][0]), np.array(times[name][1])
        step = enc + dec
        print(f"{name}: encrypt side {np.median(enc):7.2f} ms [{enc.min():.2f} .. {enc.max():.2f}], decrypt side {np.median(dec):7.2f} ms "
              f"[{dec.min():.2f} .. {dec.max():.2f}], step {np.median(step):7.2f} ms [{step.min():.2f} .. {step.max():.2f}]")


if __name__ == "__main__":
    main()
