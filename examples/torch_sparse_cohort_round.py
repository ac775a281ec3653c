#!/usr/bin/env python3
"""A sparse-job federation of ten clients simulated on ONE GPU: ten small PyTorch models in, the new global model out.

FlasheSparseCohort mirrors the sparse job's steps one to one -- sparsify (top 10 % of every layer, residuals kept in HBM per client),
the arbiter's masking choice from the clients' location lists, quantise + encrypt of the kept values with the dense aggregate of the ten
uploads, decrypt + unquantise into `out` -- with the device work of the whole cohort in a number of launches that does not grow with
the number of clients.  The result is bit for bit what ten Sparsifiers + FlasheClients produce one after the other, which this example
checks."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flashe_amd import FlasheSparseCohort, cipher as cm  # noqa: E402
from flashe_amd.block import FlasheClient, aggregate_sparse_uploads, dynamic_masking_choice  # noqa: E402
from flashe_amd.weights import Sparsifier  # noqa: E402


class Weights:
    """What the clients walk: JZFOrderDictWeights' surface (walking_order, _weights)."""

    def __init__(self, layers):
        self.walking_order = sorted(layers, key=str)
        self._weights = dict(layers)


def make_model(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 16, 5), torch.nn.ReLU(), torch.nn.Flatten(), torch.nn.Linear(16 * 28 * 28, 10)).cuda()


def main():
    cm.N_JOBS = 16                                           # every party must use the same value
    C, key, sparsity, rounds = 10, bytes(range(32)), 0.1, 2
    args = {"quantize": {"int_bits": 20, "batch": False, "element_bits": 16, "padding": True, "secure": True}, "precompute": {"enable": False},
            "mask": "dynamic"}
    models = [make_model(c) for c in range(C)]
    layers = [{name: p.detach() for name, p in m.named_parameters()} for m in models]
    names = sorted(layers[0])

    cohort = FlasheSparseCohort(args, first_idx=0, n_local=C, num_clients=C, prp_seed=key, sparsity=sparsity)
    # the same rounds as ten Sparsifiers + FlasheClients, one after the other (every client's history from the same global model)
    clients, sparsifiers = [], []
    for c in range(C):
        cl = FlasheClient(args)
        cl.create_cipher(c, C, key)
        clients.append(cl)
        sparsifiers.append(Sparsifier(sparsity))

    for it in range(rounds):
        with torch.no_grad():
            cohort.set_iter_index(it)
            enc = cohort.sparsify(layers)                    # the packed locations go to the arbiter ...
            choice = cohort.dynamic_masking()                # ... which is this process: its rule, on the device lists
            np.random.seed(it)
            upload = cohort.quantize_encrypt(normalize=True)
            new_global = {name: torch.empty_like(t) for name, t in layers[0].items()}
            cohort.decrypt_unquantize(out=new_global, unnormalize=True)
        K, total = enc.encoded[0][1], enc.encoded[0][3]
        print(f"round {it}: {C} clients, {total} parameters each, {K} kept: choice {choice!r}, path {upload.path!r}, front end {upload.front_end!r}")

        with torch.no_grad():
            masks, compact = [], []
            for sp, l in zip(sparsifiers, layers):
                w = dict(l)
                sp.sparsify(w, names)
                masks.append(sp.locations)
                compact.append(w)
            host_masks = [buf.download_at(0, np.uint32, k).astype(np.int64) for buf, k in masks]
            assert dynamic_masking_choice(host_masks, total) == choice
            np.random.seed(it)
            ups = []
            for cl, w in zip(clients, compact):
                cl.set_iter_index(it)
                cl.cipher.total = total
                cl.dynamic_masking(choice, host_masks)
                ww = Weights(w)
                ww._weights["zzz"] = np.array([0.0])
                ww.walking_order = sorted(ww._weights, key=str)
                out = cl.quantize_encrypt(ww, device=True, normalize=True)
                ups.append(out._weights[out.walking_order[0]])
            agg = aggregate_sparse_uploads(clients[0].cipher.engine, ups, host_masks, total, device=True)
            clients[0].set_idx_list(list(range(C)))
            clients[0].shape_dict = dict(sparsifiers[0].shape_dict_used_for_sparsification)
            want = {name: torch.empty_like(t) for name, t in layers[0].items()}
            clients[0].decrypt_unquantize(Weights({names[0]: agg}), out=want, unnormalize=True)
            for cl in clients[1:]:
                cl.quantizer.past_layer_mean_list = list(clients[0].quantizer.past_layer_mean_list)
                cl.quantizer.past_layer_std_list = list(clients[0].quantizer.past_layer_std_list)
        for c in range(C):
            assert upload.uploads[c].to_host().tobytes() == ups[c].to_host().tobytes(), f"client {c}'s upload differs"
        assert upload.aggregate.to_host().tobytes() == agg.to_host().tobytes()
        for name in want:
            assert torch.equal(want[name].view(torch.uint8), new_global[name].view(torch.uint8)), name
    print("uploads, aggregate and the new global model equal ten Sparsifier + FlasheClient steps bit for bit")


if __name__ == "__main__":
    main()
