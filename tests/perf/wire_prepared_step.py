#!/usr/bin/env python3
"""A precompute job's online client step to and from the packed wire form, each direction against the sequence it replaces, both from the
SAME library (the masks are the ctx's cache: prepared again, untimed, before every call, since a call consumes them):
  un-batched, int_bits 16 .. 64
    out   fused  = flashe_quantize_encrypt_prepared_pack_tensors_dev         staged = quantize_encrypt_prepared_tensors_dev + pack_dev
    back  fused  = flashe_unpack_decrypt_prepared_unquantize_model_dev       staged = unpack_dev + decrypt_prepared_unquantize_model_dev
  batched, int_bits 65 .. 128
    out   fused  = flashe_quantize_batch_encrypt_prepared_pack_model_dev     staged = quantize_batch_encrypt_prepared_model_dev + pack_dev
    back  fused  = flashe_unpack_decrypt_prepared_unbatch_unquantize_model_dev   staged = unpack_dev + decrypt_prepared_unbatch_unquantize_model_dev
Device events on the engine's stream, seven alternations of the two forms in one process, an untimed call of the same form before every
timed one, every buffer allocated outside the timed windows, parity (the packed limbs, the float64 bytes) checked inside the run.  Run it in
two processes.  Shapes: 1e7 and 25,557,032 float32 values at int_bits 20 and 64; 1,666,668 and 4,259,506 batched elements at int_bits 120
(field_bits 20).  Prints median [min .. max] per form.  The rule: a class counts as a win only where the fused median beats the staged median
by more than the larger of the two forms' spreads, in both processes."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from flashe_amd import _lib  # noqa: E402
from flashe_amd.engine import SCHEME_DOUBLE, Engine  # noqa: E402

KEY = bytes(range(32))
ROUNDS, N_JOBS, EBITS, C, IT, IDX, FB = 7, 16, 16, 10, 3, 2, 20
SIZES = [int(s) for s in os.environ.get("SIZES", "10000000,25557032").split(",")]
WIDTHS = [int(b) for b in os.environ.get("WIDTHS", "20,64").split(",")]
WIDE_SIZES = [int(s) for s in os.environ.get("WIDE_SIZES", "1666668,4259506").split(",")]
WIDE_WIDTHS = [int(b) for b in os.environ.get("WIDE_WIDTHS", "120").split(",")]


def timed(eng, prep, fn):
    prep()
    fn()                                                       # the untimed call of the same form
    prep()
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


def alternate(eng, n, n_limbs, n_out, enc, dec, out_fused, out_staged, back_fused, back_staged, bufs, title):
    pk_f, pk_s, out_f, out_s = bufs
    t = {k: [] for k in ("of", "os", "bf", "bs")}
    for _ in range(ROUNDS):
        t["of"].append(timed(eng, enc, out_fused))
        t["os"].append(timed(eng, enc, out_staged))
        t["bf"].append(timed(eng, dec, back_fused))
        t["bs"].append(timed(eng, dec, back_staged))
    assert pk_f.download(np.uint64, n_limbs).tobytes() == pk_s.download(np.uint64, n_limbs).tobytes(), "way out: parity"
    assert out_f.download(np.uint64, n_out).tobytes() == out_s.download(np.uint64, n_out).tobytes(), "way back: parity"
    print(f"{title}: parity ok", flush=True)
    print("  out")
    verdict(show("fused", t["of"]), show("staged", t["os"]))
    print("  back")
    verdict(show("fused", t["bf"]), show("staged", t["bs"]))


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
                assert eng.quantize_encrypt_prepared_pack_tensors_dev(n, rows, EBITS, du, pk_f)

            def out_staged():
                eng.quantize_encrypt_prepared_tensors_dev(n, 0, n, rows, EBITS, du, ct)
                eng.pack_dev(n, ct, pk_s)

            def back_fused():
                assert eng.unpack_decrypt_prepared_unquantize_model_dev(IT, [], [], n, N_JOBS, pk_s, back, EBITS, C, out_f)

            def back_staged():
                eng.unpack_dev(n, pk_s, el)
                eng.decrypt_prepared_unquantize_model_dev(IT, [], [], n, N_JOBS, el, back, EBITS, C, out_s)

            alternate(eng, n, n_limbs, n, lambda: eng.prepare_encrypt(IT, IDX, SCHEME_DOUBLE, n, N_JOBS), lambda: eng.prepare_decrypt(IT, C, n, N_JOBS),
                      out_fused, out_staged, back_fused, back_staged, (pk_f, pk_s, out_f, out_s), f"int_bits {b}, n = {n}")
            del xs, du, ct, pk_f, pk_s, el, out_f, out_s
        eng.prepared_discard(eng.PREPARED_ENCRYPT | eng.PREPARED_DECRYPT)
        eng.close()
    for b in WIDE_WIDTHS:
        eng = Engine(KEY, b, device=0)
        bs = b // FB
        for ne in WIDE_SIZES:
            rs = np.random.RandomState(ne % 1000 + b)
            elems = [ne // 3, ne // 3, ne - 2 * (ne // 3)]
            sizes = [e * bs - 1 for e in elems]                     # every layer's last element is padded
            alphas = [0.2, 0.15, 0.3]
            nv = sum(sizes)
            xs = [eng.upload(rs.normal(0, 0.05, s).astype(np.float32)) for s in sizes]
            du = eng.upload(rs.random_sample(nv))
            rows = [(s, x.ptr, a, False) for s, x, a in zip(sizes, xs, alphas)]
            back = [(s, None, a, False) for s, a in zip(sizes, alphas)]
            n_limbs = (ne * b + 63) // 64
            ct, pk_f, pk_s = eng.alloc_vec(ne), eng.alloc(8 * n_limbs), eng.alloc(8 * n_limbs)
            el, out_f, out_s = eng.alloc_vec(ne), eng.alloc(8 * nv), eng.alloc(8 * nv)

            def out_fused():
                assert eng.quantize_batch_encrypt_prepared_pack_model_dev(rows, EBITS, FB, du, ne, pk_f)

            def out_staged():
                eng.quantize_batch_encrypt_prepared_model_dev(rows, EBITS, FB, du, ne, ct)
                eng.pack_dev(ne, ct, pk_s)

            def back_fused():
                assert eng.unpack_decrypt_prepared_unbatch_unquantize_model_dev(IT, [], [], N_JOBS, back, EBITS, FB, C, pk_s, ne, out_f)

            def back_staged():
                eng.unpack_dev(ne, pk_s, el)
                eng.decrypt_prepared_unbatch_unquantize_model_dev(IT, [], [], N_JOBS, back, EBITS, FB, C, el, ne, out_s)

            alternate(eng, ne, n_limbs, nv, lambda: eng.prepare_encrypt(IT, IDX, SCHEME_DOUBLE, ne, N_JOBS), lambda: eng.prepare_decrypt(IT, C, ne, N_JOBS),
                      out_fused, out_staged, back_fused, back_staged, (pk_f, pk_s, out_f, out_s), f"int_bits {b} batched (field_bits {FB}), n_elems = {ne}")
            del xs, du, ct, pk_f, pk_s, el, out_f, out_s
        eng.prepared_discard(eng.PREPARED_ENCRYPT | eng.PREPARED_DECRYPT)
        eng.close()


if __name__ == "__main__":
    main()
