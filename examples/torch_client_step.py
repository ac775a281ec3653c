#!/usr/bin/env python3
"""One client's FLASHE step on a PyTorch model that lives on the GPU, without a host copy of any layer.

The model's parameters go into FlasheClient.quantize_encrypt as they are (float32 / bfloat16 / float16 / float64 tensors, read through
DLPack), and decrypt_unquantize writes the new global model straight back into them.  The client runs on torch's current stream, so the
library's kernels are ordered with the framework's own work and nothing needs an explicit synchronisation.  A single client decrypts
its own upload here; in a job the aggregate of all clients comes back from the arbiter.  flashe_amd itself never imports torch.
`--precompute` runs the precompute job: the masks are prepared while the client waits, the step adds them without AES."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flashe_amd import cipher as cm  # noqa: E402
from flashe_amd.block import FlasheClient  # noqa: E402


class Weights:
    """What the client walks: JZFOrderDictWeights' surface (walking_order, _weights)."""

    def __init__(self, layers):
        self.walking_order = sorted(layers)
        self._weights = dict(layers)


def main():
    cm.N_JOBS = 16                                           # every party must use the same value
    model = torch.nn.Sequential(torch.nn.Conv2d(3, 16, 5), torch.nn.ReLU(), torch.nn.Flatten(), torch.nn.Linear(16 * 28 * 28, 10)).cuda()
    params = {name: p for name, p in model.named_parameters()}
    # --precompute: the paper's own configuration -- the masks of the next round are computed while the client waits for the aggregate
    # (prepare_encrypt / prepare_decrypt), and the step itself then runs no AES at all
    precompute = "--precompute" in sys.argv
    num_params = sum(p.numel() for p in params.values())
    args = {"quantize": {"int_bits": 128, "batch": False, "element_bits": 16, "padding": True, "secure": True},
            "precompute": {"enable": precompute, "num_params": num_params}}
    client = FlasheClient(args, stream=torch.cuda.current_stream().cuda_stream)
    client.create_cipher(0, 1, bytes(range(32)))             # (with precompute: also the masks of round 0)
    for it in range(3):
        client.set_iter_index(it)
        with torch.no_grad():                                # (a tensor that requires grad cannot be exported)
            upload = client.quantize_encrypt(Weights({k: p.detach() for k, p in params.items()}), device=True, normalize=True)
            client.prepare_encrypt()                         # no-ops without precompute: the next round's masks, then this one's
            client.prepare_decrypt()                         # decrypt masks, while the arbiter aggregates
            client.set_idx_list([0])
            out = {k: p.detach() for k, p in params.items()}
            client.decrypt_unquantize(upload, out=out, unnormalize=True)
        q = client.quantizer
        print(f"round {it}: layer means {[f'{float(m):+.5f}' for m in q.past_layer_mean_list]}, "
              f"stds {[f'{float(s):.5f}' for s in q.past_layer_std_list]}")
    print("weights updated in place:", all(np.isfinite(p.detach().float().cpu().numpy()).all() for p in params.values()))


if __name__ == "__main__":
    main()
