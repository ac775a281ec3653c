#!/usr/bin/env python3
"""The SPARSE job's way back from the packed wire form (single mask, un-batched, int_bits 16 .. 64), against the sequence it replaces, both
from the SAME library and with the same bounds handle:
  fused = flashe_unpack_sparse_decrypt_unquantize_model_dev      staged = unpack_dev + sparse_decrypt_dev(bounds=) + unquantize_model_dev
The method of wire_client_step.py: device events on the engine's stream, seven alternations of the two forms in one process, an untimed
call of the same form before every timed one, every buffer allocated outside the timed windows, parity (the float64 bytes) checked inside
the run.  Shapes: 25,557,032 positions with 50 clients at 1 % each (config 5) and with 10 clients at 10 % (the s100_dyn jobs' sparsity),
1e7 positions with 10 clients at 10 %; int_bits 20 and 64; three layers.  The rule: a class takes the fused launch only where its median
beats the staged median by more than the larger of the two forms' spreads -- in every process it is run in."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flashe_amd.engine import Engine  # noqa: E402
from wire_client_step import show, timed, verdict  # noqa: E402

KEY = bytes(range(32))
ROUNDS, N_JOBS, EBITS, IT = 7, 16, 16, 3
SHAPES = [tuple(float(v) for v in s.split("/")) for s in os.environ.get("SHAPES", "25557032/50/0.01,25557032/10/0.1,10000000/10/0.1").split(",")]
WIDTHS = [int(w) for w in os.environ.get("WIDTHS", "20,64").split(",")]


def sparse_list(rs, total, p):
    """strictly increasing positions at density p: the running sum of geometric gaps"""
    at = np.cumsum(rs.geometric(p, int(total * p * 1.1) + 16)) - 1
    return at[at < total].astype(np.uint32)


def main():
    for b in WIDTHS:
        eng = Engine(KEY, b, device=0)
        for total, C, p in SHAPES:
            total, C = int(total), int(C)
            rs = np.random.RandomState(total % 1000 + b + C)
            locs = [sparse_list(rs, total, p) for _ in range(C)]
            ks = [int(l.size) for l in locs]
            dl = [eng.upload(l) for l in locs]
            bnd = eng.span_bounds(total, dl, ks)
            n_limbs = (total * b + 63) // 64
            limbs = rs.randint(0, 1 << 32, 2 * n_limbs, dtype=np.uint32).view(np.uint64)
            if total * b % 64:
                limbs[-1] &= np.uint64((1 << (total * b % 64)) - 1)
            pk, el, dec, out_f, out_s = eng.upload(limbs), eng.alloc_vec(total), eng.alloc_vec(total), eng.alloc(8 * total), eng.alloc(8 * total)
            sizes = [total // 3, total // 3]
            back = [(s, None, a, False) for s, a in zip([0, sizes[0], sizes[0] + sizes[1]], [0.2, 0.15, 0.3])]

            def fused():
                assert eng.unpack_sparse_decrypt_unquantize_model_dev(IT, dl, ks, total, N_JOBS, pk, back, EBITS, C, out_f, bounds=bnd)

            def staged():
                eng.unpack_dev(total, pk, el)
                eng.sparse_decrypt_dev(IT, dl, ks, total, N_JOBS, el, dec, sorted_lists=True, bounds=bnd)
                eng.unquantize_model_dev(total, 0, total, dec, back, EBITS, C, out_s)

            t = {"f": [], "s": []}
            for _ in range(ROUNDS):
                t["f"].append(timed(eng, fused))
                t["s"].append(timed(eng, staged))
            assert out_f.download(np.uint64, total).tobytes() == out_s.download(np.uint64, total).tobytes(), "way back: parity"
            print(f"int_bits {b}, total = {total} positions, {C} clients at {p:g} ({sum(ks)} entries): parity ok", flush=True)
            verdict(show("fused", t["f"]), show("staged", t["s"]))
            del pk, el, dec, out_f, out_s, dl, bnd
        eng.close()


if __name__ == "__main__":
    main()
