#!/usr/bin/env python3
"""The dense client step to and from the packed wire form, each direction against the sequence it replaces, both from the SAME library:
  out   fused  = flashe_quantize_encrypt_pack_tensors_dev            staged = quantize_encrypt_tensors_dev + pack_dev
  back  fused  = flashe_unpack_decrypt_unquantize_model_dev          staged = unpack_dev + decrypt_unquantize_model_dev
Device events on the engine's stream, seven alternations of the two forms in one process, an untimed call of the same form before every
timed one, every buffer allocated outside the timed windows, parity (the packed limbs, the float64 bytes) checked inside the run.
Shapes: 1e7 and 25,557,032 float32 values at int_bits 20, 23 and 64, double mask.  Prints median [min .. max] per form and the bytes
moved per value by DESIGN.md 4's counts.  The rule (round 9's): a (direction, width) takes the fused launch only where its median beats
the staged median by more than the larger of the two forms' spreads."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flashe_amd import _lib  # noqa: E402
from flashe_amd.engine import SCHEME_DOUBLE, Engine  # noqa: E402

KEY = bytes(range(32))
ROUNDS, N_JOBS, EBITS, C, IT, IDX = 7, 16, 16, 10, 3, 2
SIZES = [int(s) for s in os.environ.get("SIZES", "10000000,25557032").split(",")]
WIDTHS = [int(b) for b in os.environ.get("WIDTHS", "20,23,64").split(",")]


def timed(eng, fn):
    fn()                                                       # the untimed call of the same form
    a, b = eng.event(), eng.event()
    eng.record(a)
    fn()
    eng.record(b)
    eng.sync()
    ms = eng.elapsed_ms(a, b)
    eng.event_destroy(a)
    eng.event_destroy(b)
    return ms


def show(name, ts):
    ts = sorted(ts)
    print(f"    {name:<7s} {ts[len(ts) // 2]:8.3f} ms [{ts[0]:.3f} .. {ts[-1]:.3f}]", flush=True)
    return ts[len(ts) // 2], ts[-1] - ts[0]


def verdict(f, s):
    win = s[0] - f[0] > max(f[1], s[1])
    print(f"    -> {'FUSED' if win else 'staged'}: staged / fused = {s[0] / f[0]:.3f}", flush=True)


def main():
    for b in WIDTHS:
        eng = Engine(KEY, b, device=0)
        for n in SIZES:
            rs = np.random.RandomState(n % 1000 + b)
            sizes = [n // 3, n // 3, n - 2 * (n // 3)]
            starts = [0, sizes[0], sizes[0] + sizes[1]]
            alphas = [0.2, 0.15, 0.3]
            xs = [eng.upload(rs.normal(0, 0.05, s).astype(np.float32)) for s in sizes]
            du = eng.upload(rs.random_sample(n))
            rows = [(s, x.ptr, a, 0.0, _lib.TENSOR_F32, 0) for s, x, a in zip(starts, xs, alphas)]
            back = [(s, None, a, False) for s, a in zip(starts, alphas)]
            n_limbs = (n * b + 63) // 64
            ct, pk_f, pk_s = eng.alloc(8 * n), eng.alloc(8 * n_limbs), eng.alloc(8 * n_limbs)
            el, out_f, out_s = eng.alloc(8 * n), eng.alloc(8 * n), eng.alloc(8 * n)

            def out_fused():
                assert eng.quantize_encrypt_pack_tensors_dev(IT, IDX, SCHEME_DOUBLE, n, N_JOBS, rows, EBITS, du, pk_f)

            def out_staged():
                eng.quantize_encrypt_tensors_dev(IT, IDX, SCHEME_DOUBLE, n, N_JOBS, 0, n, rows, EBITS, du, ct)
                eng.pack_dev(n, ct, pk_s)

            def back_fused():
                assert eng.unpack_decrypt_unquantize_model_dev(IT, [IDX + 1], [IDX], n, N_JOBS, pk_s, back, EBITS, C, out_f)

            def back_staged():
                eng.unpack_dev(n, pk_s, el)
                eng.decrypt_unquantize_model_dev(IT, [IDX + 1], [IDX], n, N_JOBS, 0, n, el, back, EBITS, C, out_s)

            t = {k: [] for k in ("of", "os", "bf", "bs")}
            for _ in range(ROUNDS):
                t["of"].append(timed(eng, out_fused))
                t["os"].append(timed(eng, out_staged))
                t["bf"].append(timed(eng, back_fused))
                t["bs"].append(timed(eng, back_staged))
            assert pk_f.download(np.uint64, n_limbs).tobytes() == pk_s.download(np.uint64, n_limbs).tobytes(), "way out: parity"
            assert out_f.download(np.uint64, n).tobytes() == out_s.download(np.uint64, n).tobytes(), "way back: parity"
            print(f"int_bits {b}, n = {n}: parity ok", flush=True)
            print(f"  out   bytes per value: fused {12 + 2 * b / 8:.1f} (4 + 8 + {b / 8:.1f} written + {b / 8:.1f} cleared), staged {28 + b / 8:.1f}")
            verdict(show("fused", t["of"]), show("staged", t["os"]))
            print(f"  back  bytes per value: fused {8 + b / 8:.1f}, staged {24 + b / 8:.1f}")
            verdict(show("fused", t["bf"]), show("staged", t["bs"]))
            del xs, du, ct, pk_f, pk_s, el, out_f, out_s
        eng.close()


if __name__ == "__main__":
    main()
