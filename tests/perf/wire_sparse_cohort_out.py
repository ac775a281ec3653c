#!/usr/bin/env python3
"""A sparse cohort's uploads from the floats to their packed wire form (int_bits 16 .. 64), against the sequence it replaces, both from the
SAME library on the same draws:
  fused  = flashe_quantize_encrypt_pack_sparse_cohort_dev (the one clearing fill + prf_small_pack_cohort_kernel)
  staged = today's front end -- flashe_quantize_encrypt_sparse_cohort_dev, the chained launch, where it exists (int_bits 16 / 20 / 23 / 24 /
           32), else flashe_quantize_cohort_dev + one encrypt_dev(SINGLE) per client -- followed by C pack_dev
The method of wire_sparse_agg.py: device events on the engine's stream, seven alternations of the two forms in one process, an untimed
call of the same form before every timed one, every buffer allocated outside the timed windows, parity (every limb of every upload, the
zeros) checked inside the run.  Both forms upload their tables synchronously inside the window.  Shapes: ten clients at K = 2,555,703
(ResNet-50 at sparsity 0.1), fifty at K = 255,570 (config 5), ten at K = 1,000,000; int_bits 20 and 64.  The rule: packed=True takes the
fused launch only if its median beats the staged median by more than the larger of the two forms' spreads in every class -- in every
process it is run in."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flashe_amd import _lib  # noqa: E402
from flashe_amd.engine import SCHEME_SINGLE, Engine  # noqa: E402
from wire_client_step import show, timed, verdict  # noqa: E402

KEY = bytes(range(32))
ROUNDS, IT, N_JOBS, EBITS = 7, 3, 16, 16
SHAPES = [tuple(int(v) for v in s.split("/")) for s in os.environ.get("SHAPES", "10/2555703,50/255570,10/1000000").split(",")]
WIDTHS = [int(w) for w in os.environ.get("WIDTHS", "20,64").split(",")]


def main():
    for b in WIDTHS:
        eng = Engine(KEY, b, device=0)
        for C, K in SHAPES:
            rs = np.random.RandomState(K % 1000 + b + C)
            sizes = [K // 3, K // 3, K - 2 * (K // 3)]
            starts, alphas = [0, sizes[0], sizes[0] + sizes[1]], [0.2, 0.15, 0.3]
            rows = [(s, None, a, 0.0, _lib.TENSOR_F32, 0) for s, a in zip(starts, alphas)]
            xs = [[eng.upload(rs.normal(0, 0.05, s).astype(np.float32)) for s in sizes] for _ in range(C)]
            srcs, dts = [[x.ptr for x in row] for row in xs], [[_lib.TENSOR_F32] * 3] * C
            du, zzz, idx = eng.upload(rs.random_sample(C * (K + 1))), [0.0] * C, list(range(C))
            n_limbs = ((K + 1) * b + 63) // 64
            stride = (n_limbs + 1) & ~1
            pk_f, pk_s = eng.alloc(8 * C * stride), [eng.alloc(8 * n_limbs) for _ in range(C)]
            ups, pts = [eng.alloc_vec(K + 1) for _ in range(C)], [eng.alloc_vec(K) for _ in range(C)]
            z_f, z_s = eng.alloc(8 * C + 16), eng.alloc(8 * C + 16)

            def fused():
                assert eng.quantize_encrypt_pack_sparse_cohort_dev(IT, idx, K, N_JOBS, rows, srcs, dts, EBITS, du, K + 1, zzz, True, pk_f, stride, z_f)

            def staged():
                if not eng.quantize_encrypt_sparse_cohort_dev(IT, idx, K, N_JOBS, rows, srcs, dts, EBITS, du, K + 1, zzz, True, ups, z_s):
                    eng.quantize_cohort_dev(K, rows, srcs, dts, EBITS, du, K + 1, zzz, True, pts, [u.ptr + 8 * K for u in ups], z_s)
                    for c in range(C):
                        eng.encrypt_dev(IT, idx[c], SCHEME_SINGLE, K, N_JOBS, pts[c], 1, ups[c])
                for u, p in zip(ups, pk_s):
                    eng.pack_dev(K + 1, u, p)

            t = {"f": [], "s": []}
            for _ in range(ROUNDS):
                t["f"].append(timed(eng, fused))
                t["s"].append(timed(eng, staged))
            got = pk_f.download(np.uint64, C * stride)
            for c in range(C):
                assert got[c * stride:c * stride + n_limbs].tobytes() == pk_s[c].download(np.uint64, n_limbs).tobytes(), f"upload {c}: parity"
            assert z_f.download(np.uint64, C).tobytes() == z_s.download(np.uint64, C).tobytes(), "zeros: parity"
            print(f"int_bits {b}, {C} clients at K = {K}: parity ok", flush=True)
            verdict(show("fused", t["f"]), show("staged", t["s"]))
            del xs, du, pk_f, pk_s, ups, pts
        eng.close()


if __name__ == "__main__":
    main()
