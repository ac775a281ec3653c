"""One dense round in the WIRE form: every client goes from its float model straight to the packed integer it sends
(quantize_encrypt(packed=True): one launch at int_bits 16 .. 64), the arbiter adds the packed integers where they lie, and a client takes
the packed sum back to floats in one launch.  --batch: the batched int_bits 120 job (six quantised values per element), which takes its one
launch out with packed="fused".  --precompute: a precompute job -- the masks were prepared in idle time (prepare_encrypt / prepare_decrypt),
packed="fused" adds them on the way to and from the wire form in one launch each, with no AES online.
Run on a machine with a GPU:  python examples/wire_round.py [--batch] [--precompute]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flashe_amd.block import FlasheClient  # noqa: E402

ARGS = {"quantize": {"int_bits": 20, "batch": False, "element_bits": 16, "padding": True, "secure": True},
        "precompute": {"enable": False, "num_params": None}}
SHAPES = {"conv.w": (6, 25), "fc.w": (120, 84), "fc.b": (84,)}
C = 3


class Weights:
    def __init__(self, layers):
        self.walking_order, self._weights = sorted(layers), dict(layers)


def main():
    batch, precompute = "--batch" in sys.argv[1:], "--precompute" in sys.argv[1:]
    if batch:
        ARGS["quantize"].update(int_bits=120, batch=True)
    if precompute:
        bs = 120 // (16 + int(np.ceil(np.log2(C))))
        sizes = [int(np.prod(s)) for s in SHAPES.values()]
        ARGS["precompute"] = {"enable": True, "num_params": sum((s + bs - 1) // bs for s in sizes) if batch else sum(sizes)}
    rs = np.random.RandomState(0)
    models = [{k: rs.normal(0, 0.05, s).astype(np.float32) for k, s in SHAPES.items()} for _ in range(C)]
    clients = []
    for i in range(C):
        cl = FlasheClient(ARGS)
        cl.create_cipher(i, C, bytes(range(32)))
        if precompute:                                                  # the job's order: the masks of round 1 prepared during round 0
            cl.set_iter_index(0)
            cl.prepare_encrypt()
        cl.set_iter_index(1)
        cl.quantizer.past_layer_mean_list = [np.float64(0.0)] * len(SHAPES)
        cl.quantizer.past_layer_std_list = [np.float64(0.05)] * len(SHAPES)
        clients.append(cl)
    uploads = []
    for cl, m in zip(clients, models):
        w = cl.quantize_encrypt(Weights(m), packed="fused" if batch or precompute else True)
        uploads.append(w._weights[w.walking_order[0]])                 # a PackedVector; .to_int() is what goes on the wire
    print("upload path:", uploads[0].path, "-", (uploads[0].to_int().bit_length() + 7) // 8, "bytes per client")
    total = clients[0].cipher.aggregate(uploads, packed=True)           # the arbiter: the packed integers added where they lie
    if precompute:
        clients[0].prepare_decrypt()
    clients[0].set_idx_list(list(range(C)))
    mean = clients[0].decrypt_unquantize(Weights({"sum": total}))
    want = sum(m["fc.b"].astype(np.float64) for m in models)
    print("max |error| of the summed fc.b:", float(np.abs(mean._weights["fc.b"] - want).max()))


if __name__ == "__main__":
    main()
