#!/usr/bin/env python3
"""The way back from the packed wire form with prefix LISTS (a round with a dropout, the single mask's decrypt), against the sequence it
replaces, both from the SAME library:
  un-batched  fused = flashe_unpack_decrypt_lists_unquantize_model_dev          staged = unpack_dev + decrypt_unquantize_model_dev
  batched     fused = flashe_unpack_decrypt_lists_unbatch_unquantize_model_dev  staged = unpack_dev + decrypt_dev + unbatch_unquantize_model_dev
The method of wire_client_step.py: device events on the engine's stream, seven alternations of the two forms in one process, an untimed
call of the same form before every timed one, every buffer allocated outside the timed windows, parity (the float64 bytes) checked inside
the run.  Shapes: 1e7 and 25,557,032 values in three layers; int_bits 20 and 64 un-batched, 120 / field 20 batched; prefix lists 2 + 2 (one
dropout), 4 + 4 and 0 + 10 (single mask, ten clients).  The rule: a class takes the fused launch only where its median beats the staged
median by more than the larger of the two forms' spreads -- in every process it is run in."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flashe_amd.engine import Engine  # noqa: E402
from wire_client_step import show, timed, verdict  # noqa: E402

KEY = bytes(range(32))
ROUNDS, N_JOBS, EBITS, C, IT = 7, 16, 16, 10, 3
SIZES = [int(s) for s in os.environ.get("SIZES", "10000000,25557032").split(",")]
WIDTHS = [tuple(int(v) for v in w.split("/")) for w in os.environ.get("WIDTHS", "20/0,64/0,120/20").split(",")]      # field 0: un-batched
LISTS = (([2, 5], [0, 3]), ([2, 5, 8, 11], [0, 3, 6, 9]), ([], list(range(10))))


def main():
    for b, fb in WIDTHS:
        eng, bs = Engine(KEY, b, device=0), (b // fb if fb else 1)
        for n in SIZES:
            sizes = [n // 3, n // 3, n - 2 * (n // 3)]
            alphas = [0.2, 0.15, 0.3]
            ne = sum((s + bs - 1) // bs for s in sizes)
            n_limbs = (ne * b + 63) // 64
            limbs = np.random.RandomState(n % 1000 + b).randint(0, 1 << 32, 2 * n_limbs, dtype=np.uint32).view(np.uint64)
            if ne * b % 64:
                limbs[-1] &= np.uint64((1 << (ne * b % 64)) - 1)
            pk, el, out_f, out_s = eng.upload(limbs), eng.alloc_vec(ne), eng.alloc(8 * n), eng.alloc(8 * n)
            dec = eng.alloc_vec(ne) if fb else None
            back = [(s, None, a, False) for s, a in zip(sizes if fb else [0, sizes[0], sizes[0] + sizes[1]], alphas)]
            for add, minus in LISTS:
                def fused():
                    if fb:
                        assert eng.unpack_decrypt_lists_unbatch_unquantize_model_dev(IT, add, minus, back, EBITS, fb, C, pk, ne, out_f)
                    else:
                        assert eng.unpack_decrypt_lists_unquantize_model_dev(IT, add, minus, n, N_JOBS, pk, back, EBITS, C, out_f)

                def staged():
                    eng.unpack_dev(ne, pk, el)
                    if fb:
                        eng.decrypt_dev(IT, add, minus, ne, N_JOBS, el, dec)
                        eng.unbatch_unquantize_model_dev(back, EBITS, fb, C, dec, ne, out_s)
                    else:
                        eng.decrypt_unquantize_model_dev(IT, add, minus, n, N_JOBS, 0, n, el, back, EBITS, C, out_s)

                t = {"f": [], "s": []}
                for _ in range(ROUNDS):
                    t["f"].append(timed(eng, fused))
                    t["s"].append(timed(eng, staged))
                assert out_f.download(np.uint64, n).tobytes() == out_s.download(np.uint64, n).tobytes(), "way back: parity"
                print(f"int_bits {b}, field {fb}, n = {n} values, {ne} elements, lists {len(add)} + {len(minus)}: parity ok", flush=True)
                verdict(show("fused", t["f"]), show("staged", t["s"]))
            del pk, el, dec, out_f, out_s
        eng.close()


if __name__ == "__main__":
    main()
