#!/usr/bin/env python3
"""A federation of ten clients simulated on ONE GPU: ten PyTorch models of eight million parameters in, the new global model out.

FlasheCohort takes one Weights per client (the parameters as they are, read through DLPack), runs the clients' quantise + encrypt as one
chained launch where the model is long enough to fill the chip (this one is, un-batched, on 256 CUs; shorter models take the staged
form: `upload.path` says which), and
decrypt_unquantize writes the new global model into `out`.  The result is bit for bit what ten FlasheClients produce one after the other,
which this example checks.

  --bits B     int_bits of the job (default 128; the reference's shipped un-batched jobs run 20)
  --compact    with --bits <= 32: uint32 ciphertexts and sum (FlasheCohort(compact=True)); at int_bits 16 / 20 / 23 / 24 / 32 the chained
               launch then goes from the floats to the uint32 ciphertexts
  --one-limb   with --bits 33 .. 64 (say --bits 40 or --bits 64): FlasheCohort(one_limb=True) -- the chained launch goes from the floats to
               the one-limb uint64 ciphertexts and their sum (`upload.path` is "cohort-chain"; without the flag these widths run
               "staged-chain"), no mask is kept and the decrypt of the sum takes the telescoped lists; the new global model is the same
  --batch      a batched job (the reference's *_q16_b6_pad jobs: --bits 120 --batch packs six 20-bit fields per element); the chained
               launch takes it when the model has enough batched elements to fill the chip
  --precompute a precompute job ("precompute": {"enable": true}): the cohort calls prepare_encrypt() one round ahead -- the masks of all
               ten clients as one chain of eleven PRF streams, in idle time -- and the online step is ONE launch with no AES
               (`upload.path` is "prepared-cohort"), at any --bits, with or without --compact / --batch
  --drop i,j   clients i and j miss the round (dropout-aware decrypt is what FLASHE is for): quantize_encrypt(present=...) takes the
               Weights of the clients that report, and at --bits > 64 the round is still one chained launch, over present + runs PRF
               streams, whose decrypt mask is that of the telescoped index lists; the new global model is what the present clients'
               own steps and a decrypt told who uploaded (set_idx_list(present)) give, which this example checks; with --compact at
               --bits 16 / 20 / 23 / 24 / 32 the gapped round is one chained launch too (`upload.path` is "cohort-chain"), without a mask:
               the decrypt of the sum takes the telescoped lists; and so it is with --one-limb at --bits 33 .. 64
               (--bits 40 --one-limb --drop 2,7: "cohort-chain" over eight clients' eleven PRF streams, uint64 ciphertexts)
  --cut        many clients with a SMALL model: forty LeNet-5s of 61,706 parameters, far below the length the summed chain takes uncut.
               FlasheCohort(cut=True) cuts the chain into runs of consecutive clients and adds the runs' partial sums and decrypt masks
               in one combine pass (`upload.path` is "cut-chain"): two launches instead of forty quantise passes, forty plaintext
               vectors and a batch encrypt; with --compact at --bits 16 / 20 / 23 / 24 / 32 the same in the uint32 layout.  Without
               --cut such a cohort runs "staged-chain".  With --drop 2,7 (a gap in the cipher indices is a cut the round imposes) or
               with --bits 120 --batch (five 22-bit fields per element) the example asks for FlasheCohort(cut="any"), which takes
               gapped and batched short cohorts through the cut launch too and keeps the decrypt mask of the telescoped lists
  --rng philox the stochastic-rounding draws come from one np.random.Generator per client instead of NumPy's global stream
               (quantize_encrypt(rng=[...])): counter-based Philox generators, whose draws for the whole cohort are ONE asynchronous
               launch on the device (models of 65,536 values or more: this example's hold 8,036,426) and whose advanced states come back
               -- the sequential clients below draw from identically seeded generators and must leave them in the same place;
               --rng pcg64 takes np.random.default_rng(seed) itself (PCG64, a 128-bit LCG): every lane of ONE launch jumps to its first
               draw and walks a fixed stride, and the states come back the same way; --rng sfc64 takes any other Generator: the same
               call, drawn on the host
  --inline-draws  with --precompute --bits 120 --batch --rng philox: FlasheCohort(inline_draws=True) -- the batched online launch may
               generate the Philox draws itself (no draw buffer; a lane owns four elements and computes each Philox block of their 24
               values once) in the shape classes where that form won its measurement (one shared generator at a misaligned length; this
               example's generator per client is not one), and FLASHE_INLINE_DRAWS=1 forces it;
               `upload.draws` says "inline" or "buffer", and the bytes are the same either way.  With --precompute --rng pcg64 (no
               --batch): FlasheCohort(inline_draws="any") -- the un-batched online launch may generate default_rng's PCG64 draws itself
               (a lane keeps one jump of the LCG for all clients; no draw buffer), which won its measurement in both layouts;
               FLASHE_INLINE_DRAWS=0 keeps the buffer
  --packed     a DENSE job's arbiter adds the clients' bit-packed models as one integer (carries cross from one element into the next),
               so its global model is not the decrypt of the element-wise sum: cohort.aggregate_packed() is that reduce of the upload
               -- one pass over the ciphertexts where they lie, no packed vectors -- and decrypt_unquantize(packed=True) decrypts it
               (after a chained launch still by adding the mask that launch wrote); checked against the clients' own
               cipher.aggregate(packed=True) and decrypt"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flashe_amd import cipher as cm  # noqa: E402
from flashe_amd.block import FlasheClient, FlasheCohort  # noqa: E402


class Weights:
    """What the clients walk: JZFOrderDictWeights' surface (walking_order, _weights)."""

    def __init__(self, layers):
        self.walking_order = sorted(layers)
        self._weights = dict(layers)


def make_model(seed, small=False):
    torch.manual_seed(seed)
    if small:                                                # LeNet-5 on 32 x 32 inputs: 61,706 parameters
        return torch.nn.Sequential(torch.nn.Conv2d(1, 6, 5), torch.nn.ReLU(), torch.nn.AvgPool2d(2), torch.nn.Conv2d(6, 16, 5), torch.nn.ReLU(),
                                   torch.nn.AvgPool2d(2), torch.nn.Flatten(), torch.nn.Linear(400, 120), torch.nn.ReLU(), torch.nn.Linear(120, 84),
                                   torch.nn.ReLU(), torch.nn.Linear(84, 10)).cuda()
    return torch.nn.Sequential(torch.nn.Conv2d(3, 16, 5), torch.nn.ReLU(), torch.nn.Flatten(), torch.nn.Linear(16 * 28 * 28, 640), torch.nn.ReLU(),
                               torch.nn.Linear(640, 10)).cuda()


def values(dv):
    """A DeviceVector's elements, whatever its layout (uint32 [n] compact, uint64 [n, limbs] otherwise)."""
    return np.asarray(dv.to_host(), dtype=np.uint64).reshape(len(dv), -1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--bits", type=int, default=128)
    ap.add_argument("--compact", action="store_true")
    ap.add_argument("--one-limb", action="store_true", help="with --bits 33 .. 64: the chained launch from the floats in the one-limb layout")
    ap.add_argument("--batch", action="store_true")
    ap.add_argument("--precompute", action="store_true")
    ap.add_argument("--cut", action="store_true", help="forty LeNet-sized models through the cut chained launch")
    ap.add_argument("--drop", default="", help="comma-separated clients that miss the round, e.g. 2,7")
    ap.add_argument("--packed", action="store_true", help="reduce the upload as a dense job's arbiter does: on the bit-packed integers")
    ap.add_argument("--inline-draws", action="store_true", help="a batched precompute cohort may draw its Philox stream inside the online launch; with --rng pcg64: inline_draws=\"any\"")
    ap.add_argument("--rng", choices=["philox", "pcg64", "sfc64"], default=None, help="draw from one np.random.Generator per client")
    opt = ap.parse_args()
    cm.N_JOBS = 16                                           # every party must use the same value
    C, key = 40 if opt.cut else 10, bytes(range(32))
    dropped = sorted({int(c) for c in opt.drop.split(",") if c})
    present = [c for c in range(C) if c not in dropped]
    models = [make_model(c, small=opt.cut) for c in range(C)]
    layers = [{name: p.detach() for name, p in m.named_parameters()} for m in models]
    # a precompute job states the length of its uploads: the values of the model, or -- batched -- its elements of bs values, every layer
    # padded to whole elements on its own
    eb = min(16, opt.bits - int(np.ceil(np.log2(C)))) if opt.cut else 16          # (forty clients: their sum must still fit int_bits)
    bs = opt.bits // (eb + int(np.ceil(np.log2(C)))) if opt.batch else 1
    num_params = sum((t.numel() + bs - 1) // bs for t in layers[0].values())
    args = {"quantize": {"int_bits": opt.bits, "batch": opt.batch, "element_bits": eb, "padding": True, "secure": True},
            "precompute": {"enable": opt.precompute, "num_params": num_params}}
    it = 1 if opt.precompute else 0

    def generators():
        """One Generator per present client, seeded alike on both sides (None: NumPy's global stream, seeded below)."""
        if opt.rng is None:
            return None
        if opt.rng == "pcg64":
            return [np.random.default_rng(1000 + c) for c in present]
        bitgen = np.random.Philox if opt.rng == "philox" else np.random.SFC64
        return [np.random.Generator(bitgen(1000 + c)) for c in present]

    cohort = FlasheCohort(args, first_idx=0, n_local=C, num_clients=C, prp_seed=key, compact=opt.compact, one_limb=opt.one_limb,
                          cut="any" if opt.cut and (dropped or opt.batch) else opt.cut, inline_draws="any" if opt.inline_draws and opt.rng == "pcg64" else opt.inline_draws)
    if opt.precompute:
        cohort.set_iter_index(it - 1)
        cohort.prepare_encrypt()                             # in idle time, one round ahead: the masks of iteration `it`
    cohort.set_iter_index(it)
    np.random.seed(0)
    with torch.no_grad():
        gens = generators()
        upload = cohort.quantize_encrypt([Weights(layers[c]) for c in present], normalize=True, present=present if dropped else None, rng=gens)
        new_global = {name: torch.empty_like(t) for name, t in layers[0].items()}
        packed_sum = cohort.aggregate_packed() if opt.packed else None
        cohort.decrypt_unquantize(out=new_global, unnormalize=True, packed=opt.packed)
    print(f"{C} clients{f' of which {dropped} dropped out' if dropped else ''}, {sum(t.numel() for t in layers[0].values())} parameters each: path {upload.path!r}, "
          f"{len(upload.ciphertexts)} ciphertexts and their sum in HBM ({upload.partial_sum.elem_bytes * upload.partial_sum.limbs} bytes per element), draws {upload.draws!r}")

    # the same round as the present FlasheClients, one after the other
    clients = []
    for c in range(C):
        cl = FlasheClient(args)
        cl.create_cipher(c, C, key)
        if opt.precompute:
            cl.set_iter_index(it - 1)
            cl.prepare_encrypt()                             # every client its own two mask vectors
        cl.set_iter_index(it)
        clients.append(cl)
    np.random.seed(0)
    with torch.no_grad():
        cts, twins = [], generators()
        for p, c in enumerate(present):
            w = clients[c].quantize_encrypt(Weights(layers[c]), device=True, normalize=True, rng=twins[p] if twins else None)
            cts.append(w._weights[w.walking_order[0]])
        lead = clients[present[0]]
        agg_elem = lead.cipher.aggregate(cts)
        agg = lead.cipher.aggregate(cts, packed=True) if opt.packed else agg_elem
        lead.set_idx_list(list(present))                     # who uploaded: the decrypt telescopes the runs of indices
        want = {name: torch.empty_like(t) for name, t in layers[0].items()}
        lead.decrypt_unquantize(Weights({sorted(layers[0])[0]: agg}), out=want, unnormalize=True)
    assert upload.present == present
    for p, c in enumerate(present):
        assert np.array_equal(values(upload.ciphertexts[p]), values(cts[p])), f"client {c}'s upload differs"
    assert np.array_equal(values(upload.partial_sum), values(agg_elem))
    if opt.packed:
        assert np.array_equal(values(packed_sum), values(agg))
        print(f"packed reduce: {int((values(packed_sum) != values(agg_elem)).any(axis=1).sum())} of {len(packed_sum)} elements differ from the element-wise sum by a carry")
    if gens:                                                 # the cohort handed every generator back where its client's own step leaves it
        assert all(a.random() == b.random() for a, b in zip(gens, twins))
    for name in want:
        assert torch.equal(want[name].view(torch.uint8), new_global[name].view(torch.uint8)), name
    if dropped:
        print(f"new global model equals {len(present)} FlasheClient steps and their dropout-aware decrypt bit for bit")
        return
    last = list(layers[0])[-1]                               # the last layer's bias ("5.bias"; "11.bias" of the small model)
    mean = sum(l[last].double() for l in layers) / C
    print(f"new global model equals {C} FlasheClient steps bit for bit; |{last} - mean of the clients'| <=",
          float((new_global[last].double() - mean).abs().max()))


if __name__ == "__main__":
    main()
