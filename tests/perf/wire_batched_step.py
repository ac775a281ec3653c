#!/usr/bin/env python3
"""The BATCHED client step to and from the packed wire form (int_bits 65 .. 128), each direction against the sequence it replaces, both
from the SAME library:
  out   fused  = flashe_quantize_batch_encrypt_pack_model_dev            staged = quantize_batch_model_dev + encrypt_dev + pack_dev
  back  fused  = flashe_unpack_decrypt_unbatch_unquantize_model_dev      staged = unpack_dev + decrypt_dev + unbatch_unquantize_model_dev
Device events on the engine's stream, seven alternations of the two forms in one process, an untimed call of the same form before every
timed one, every buffer allocated outside the timed windows, parity (the packed limbs, the float64 bytes) checked inside the run.
Shapes: 61,706, 1e7 and 25,557,032 float32 values (and three sizes between, which place the way back's threshold) in three layers at int_bits 120 / field 20 and int_bits 128 / field 21, double mask.
Prints median [min .. max] per form and the bytes moved per batched element by the launches' signatures.  The rule: a (direction, shape)
takes the fused launch only where its median beats the staged median by more than the larger of the two forms' spreads."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flashe_amd.engine import SCHEME_DOUBLE, Engine  # noqa: E402
from wire_client_step import show, timed, verdict  # noqa: E402

KEY = bytes(range(32))
ROUNDS, N_JOBS, EBITS, C, IT, IDX = 7, 16, 16, 10, 3, 2
SIZES = [int(s) for s in os.environ.get("SIZES", "61706,300000,1000000,3000000,10000000,25557032").split(",")]
WIDTHS = [tuple(int(v) for v in w.split("/")) for w in os.environ.get("WIDTHS", "120/20,128/21").split(",")]


def main():
    for b, fb in WIDTHS:
        eng, bs = Engine(KEY, b, device=0), b // fb
        for n in SIZES:
            rs = np.random.RandomState(n % 1000 + b)
            sizes = [n // 3, n // 3, n - 2 * (n // 3)]
            alphas = [0.2, 0.15, 0.3]
            xs = [eng.upload(rs.normal(0, 0.05, s).astype(np.float32)) for s in sizes]
            du = eng.upload(rs.random_sample(n))
            rows = [(s, x.ptr, a, False) for s, x, a in zip(sizes, xs, alphas)]
            back = [(s, None, a, False) for s, a in zip(sizes, alphas)]
            ne = sum((s + bs - 1) // bs for s in sizes)
            n_limbs = (ne * b + 63) // 64
            pt, ct, pk_f, pk_s = eng.alloc_vec(ne), eng.alloc_vec(ne), eng.alloc(8 * n_limbs), eng.alloc(8 * n_limbs)
            el, dec, out_f, out_s = eng.alloc_vec(ne), eng.alloc_vec(ne), eng.alloc(8 * n), eng.alloc(8 * n)

            def out_fused():
                assert eng.quantize_batch_encrypt_pack_model_dev(IT, IDX, SCHEME_DOUBLE, rows, EBITS, fb, du, ne, pk_f)

            def out_staged():
                eng.quantize_batch_model_dev(rows, EBITS, fb, du, ne, pt)
                eng.encrypt_dev(IT, IDX, SCHEME_DOUBLE, ne, N_JOBS, pt, eng.limbs, ct)
                eng.pack_dev(ne, ct, pk_s)

            def back_fused():
                assert eng.unpack_decrypt_unbatch_unquantize_model_dev(IT, [IDX + 1], [IDX], back, EBITS, fb, C, pk_s, ne, out_f)

            def back_staged():
                eng.unpack_dev(ne, pk_s, el)
                eng.decrypt_dev(IT, [IDX + 1], [IDX], ne, N_JOBS, el, dec)
                eng.unbatch_unquantize_model_dev(back, EBITS, fb, C, dec, ne, out_s)

            t = {k: [] for k in ("of", "os", "bf", "bs")}
            for _ in range(ROUNDS):
                t["of"].append(timed(eng, out_fused))
                t["os"].append(timed(eng, out_staged))
                t["bf"].append(timed(eng, back_fused))
                t["bs"].append(timed(eng, back_staged))
            assert pk_f.download(np.uint64, n_limbs).tobytes() == pk_s.download(np.uint64, n_limbs).tobytes(), "way out: parity"
            assert out_f.download(np.uint64, n).tobytes() == out_s.download(np.uint64, n).tobytes(), "way back: parity"
            print(f"int_bits {b}, field {fb}, n = {n} values, {ne} elements: parity ok", flush=True)
            print(f"  out   bytes per element: fused {12 * bs + b / 8:.0f}, staged {12 * bs + 64 + b / 8:.0f}")
            verdict(show("fused", t["of"]), show("staged", t["os"]))
            print(f"  back  bytes per element: fused {8 * bs + b / 8:.0f}, staged {8 * bs + 64 + b / 8:.0f}")
            verdict(show("fused", t["bf"]), show("staged", t["bs"]))
            del xs, du, pt, ct, pk_f, pk_s, el, dec, out_f, out_s
        eng.close()


if __name__ == "__main__":
    main()
