#!/usr/bin/env python3
"""One client's FLASHE step on a PyTorch model that lives on the GPU, without a host copy of any layer.

The model's parameters go into FlasheClient.quantize_encrypt as they are (float32 / bfloat16 / float16 / float64 tensors, read through
DLPack), and decrypt_unquantize writes the new global model straight back into them.  The client runs on torch's current stream, so the
library's kernels are ordered with the framework's own work and nothing needs an explicit synchronisation.  A single client decrypts
its own upload here; in a job the aggregate of all clients comes back from the arbiter.  flashe_amd itself never imports torch.
`--precompute` runs the precompute job: the masks are prepared while the client waits, the step adds them without AES.
`--degree D --total-degree T` weights the model by the client's sample count as the aggregator does (jzf_aggregator.py:676, :902-907):
the multiply rides the stage pass, the two divisions and the add of the last round's model ride the store pass, the parameters are
updated in place; every round is checked against the same sequence written out with NumPy on host copies."""
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


def _option(name):
    """The float behind `name` on the command line, None without it."""
    return float(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else None


def _host_round(client, host, it, degree, total, seed):
    """The reference's sequence on host copies: weights *= degree, the step, / (total / degree), unnormalize, / degree, + last round."""
    client.set_iter_index(it)
    np.random.seed(seed)
    upload = client.quantize_encrypt(Weights({k: v * degree for k, v in host.items()}), device=True, normalize=True)
    client.set_idx_list([0])
    w = client.decrypt_unquantize(upload)
    for k in w.walking_order:
        w._weights[k] = w._weights[k] / (total / degree)
    w = client.unnormalize(w)
    return {k: (host[k] + w._weights[k] / degree).astype(np.float32) for k in w.walking_order}


def main():
    cm.N_JOBS = 16                                           # every party must use the same value
    degree, total = _option("--degree"), _option("--total-degree")
    if (degree is None) != (total is None):
        sys.exit("--degree and --total-degree come together")
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
    if degree is not None:
        twin = FlasheClient(dict(args, precompute={"enable": False}))        # the written-out sequence runs beside the fused step
        twin.create_cipher(0, 1, bytes(range(32)))
    for it in range(3):
        client.set_iter_index(it)
        with torch.no_grad():                                # (a tensor that requires grad cannot be exported)
            if degree is not None:
                want = _host_round(twin, {k: p.detach().cpu().numpy() for k, p in params.items()}, it, degree, total, seed=it)
                np.random.seed(it)
                out = {k: p.detach() for k, p in params.items()}
                upload = client.quantize_encrypt(Weights(dict(out)), device=True, normalize=True, degree=degree)
                client.prepare_encrypt()
                client.prepare_decrypt()
                client.set_idx_list([0])
                client.decrypt_unquantize(upload, out=out, unnormalize=True, total_degree=total, last_round=out)     # in place
                same = all(p.detach().cpu().numpy().tobytes() == want[k].tobytes() for k, p in params.items())
                same = same and [float(m).hex() for m in client.quantizer.past_layer_mean_list] == [float(m).hex() for m in twin.quantizer.past_layer_mean_list]
                print(f"round {it}: degree {degree:g} of {total:g}, equal to the written-out host sequence: {same}")
                continue
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
