#!/usr/bin/env python3
"""The arbiter's side of the SPARSE job on the packed wire form (int_bits 16 .. 64), against the sequence it replaces, both from the SAME
library and with the same bounds handle:
  fused = flashe_sparse_aggregate_packed_dev      staged = C unpack_dev + sparse_aggregate_dev(bounds=) + pack_dev
The staged form is given the zeros up front: the C synchronous downloads block.aggregate_sparse_uploads pays for them are NOT in its time.
The method of wire_client_step.py: device events on the engine's stream, seven alternations of the two forms in one process, an untimed
call of the same form before every timed one, every buffer allocated outside the timed windows, parity (the limbs) checked inside the
run.  Shapes: 25,557,032 positions with 50 clients at 1 % each (config 5) and with 10 clients at 10 %, 1e7 positions with 10 clients at
10 %; int_bits 20 and 64.  The rule: the fused launch becomes the default only if its median beats the staged median by more than the
larger of the two forms' spreads in every class -- in every process it is run in."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flashe_amd.engine import Engine  # noqa: E402
from wire_client_step import show, timed, verdict  # noqa: E402
from wire_sparse_back import sparse_list  # noqa: E402

KEY = bytes(range(32))
ROUNDS = 7
SHAPES = [tuple(float(v) for v in s.split("/")) for s in os.environ.get("SHAPES", "25557032/50/0.01,25557032/10/0.1,10000000/10/0.1").split(",")]
WIDTHS = [int(w) for w in os.environ.get("WIDTHS", "20,64").split(",")]


def random_limbs(rs, n, b):
    """the limbs of a random integer of n b-bit fields"""
    limbs = rs.randint(0, 1 << 32, 2 * ((n * b + 63) // 64), dtype=np.uint32).view(np.uint64)
    if n * b % 64:
        limbs[-1] &= np.uint64((1 << (n * b % 64)) - 1)
    return limbs


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
            ups = [random_limbs(rs, k + 1, b) for k in ks]
            zeros = [[int(u[0]) & ((1 << b) - 1)] for u in ups]
            pk = [eng.upload(u) for u in ups]
            el = [eng.alloc_vec(k + 1) for k in ks]
            n_limbs = (total * b + 63) // 64
            dense, out_f, out_s = eng.alloc_vec(total), eng.alloc(8 * n_limbs), eng.alloc(8 * n_limbs)

            def fused():
                assert eng.sparse_aggregate_packed_dev(total, dl, ks, pk, out_f, bounds=bnd)

            def staged():
                for k, src, dst in zip(ks, pk, el):
                    eng.unpack_dev(k + 1, src, dst)
                eng.sparse_aggregate_dev(total, dl, ks, el, zeros, dense, sorted_lists=True, bounds=bnd)
                eng.pack_dev(total, dense, out_s)

            t = {"f": [], "s": []}
            for _ in range(ROUNDS):
                t["f"].append(timed(eng, fused))
                t["s"].append(timed(eng, staged))
            assert out_f.download(np.uint64, n_limbs).tobytes() == out_s.download(np.uint64, n_limbs).tobytes(), "packed sum: parity"
            print(f"int_bits {b}, total = {total} positions, {C} clients at {p:g} ({sum(ks)} entries): parity ok", flush=True)
            verdict(show("fused", t["f"]), show("staged", t["s"]))
            del pk, el, dense, out_f, out_s, dl, bnd
        eng.close()


if __name__ == "__main__":
    main()
