#!/usr/bin/env python3
"""The arbiter's packed reduce of ciphertexts that lie UNPACKED in HBM, two forms on the same operands, alternated in one process:

  elems   flashe_aggregate_packed_elems_dev / _u32_dev: one pass over the unpacked vectors (two launches: the scan and the look-back);
  parent  what cipher.aggregate(packed=True) ran before that call existed: (compact operands: C widens,) C pack_dev launches into C packed
          temporaries, aggregate_packed_dev (two launches), unpack_dev.

HIP-event times of `--calls` back-to-back calls per window, `--rounds` windows per form in the order elems, parent, elems, parent, ...; the
windows of ONE form are its repeats, their spread is the run-to-run spread the difference is judged against.  Every buffer of both forms
is allocated once, outside the windows (the parent's form allocates its temporaries per call in cipher.aggregate: not counted here).  The
two results are compared on the host before anything is timed.  Bytes per form are computed from the shapes.

Sizes: config 2 (n = 1e7, int_bits 128, C = 10) and the shipped jobs' shape (n = 25,557,032, int_bits 20, C = 10, compact uint32 operands).
usage: packed_elems_reduce.py [--rounds R] [--calls K] [--scale S]     (--scale 0.01: a rehearsal at a hundredth of the lengths)"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SIZES = [("config 2", 10_000_000, 128, 10, False), ("shipped jobs", 25_557_032, 20, 10, True)]


def bytes_moved(n, b, C, compact):
    """(elems, parent, parent's temporaries) in bytes, from the shapes."""
    eb = 4 if compact else 16 if b > 64 else 8
    wide = 16 if b > 64 else 8                      # the layout the parent's pack reads and its unpack writes
    packed = (n * b + 63) // 64 * 8
    elems = (C + 1) * n * eb
    widen = C * n * (4 + 8) if compact else 0
    parent = widen + C * (n * wide + packed) + (C + 1) * packed + packed + n * wide
    temps = (C * n * 8 if compact else 0) + (C + 1) * packed
    return elems, parent, temps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--scale", type=float, default=1.0)
    a = ap.parse_args()
    from flashe_amd.engine import Engine
    for name, n, b, C, compact in SIZES:
        n = max(int(n * a.scale), 1)
        eng = Engine(bytes(range(32)), b)
        limbs = 2 if b > 64 else 1
        rng = np.random.Generator(np.random.PCG64(b))
        if compact:
            host = [rng.integers(0, 1 << b, n, dtype=np.uint32) for _ in range(C)]
        else:
            host = [rng.integers(0, 2 ** 64, (n, limbs), dtype=np.uint64) for _ in range(C)]
            if b % 64:
                for h in host:
                    h[:, -1] &= np.uint64((1 << (b % 64)) - 1)
        ops = [eng.upload(h) for h in host]
        n_limbs = (n * b + 63) // 64
        out_new = eng.alloc(max(n * (4 if compact else 8 * limbs), 16))
        wide = [eng.alloc_vec(n, 1) for _ in range(C)] if compact else ops
        packed = [eng.alloc(max(n_limbs * 8, 16)) for _ in range(C)]
        psum, out_old = eng.alloc(max(n_limbs * 8, 16)), eng.alloc_vec(n, limbs)

        def elems():
            took = eng.aggregate_packed_elems_u32_dev(ops, n, out_new) if compact else eng.aggregate_packed_elems_dev(ops, n, out_new)
            assert took

        def parent():
            if compact:
                for s, w in zip(ops, wide):
                    eng.widen_u32_dev(n, s, w)
            for s, p in zip(wide, packed):
                eng.pack_dev(n, s, p)
            eng.aggregate_packed_dev(packed, n_limbs, n * b, psum)
            eng.unpack_dev(n, psum, out_old)

        elems()
        parent()
        eng.sync()
        got = out_new.download(np.uint32 if compact else np.uint64, n * (1 if compact else limbs)).astype(np.uint64)
        want = out_old.download(np.uint64, n * limbs)
        assert np.array_equal(got, want), "the two forms disagree"
        elem_sum = np.zeros(n * limbs, dtype=np.uint64)
        if limbs == 1:
            for h in host:
                elem_sum += h.reshape(-1).astype(np.uint64)
            carried = int(np.count_nonzero((elem_sum & np.uint64((1 << b) - 1 if b < 64 else 2 ** 64 - 1)) != want))
        else:
            carried = -1
        forms = {"elems": elems, "parent": parent}
        for f in forms.values():                    # warm-up of both forms at this shape
            for _ in range(5):
                f()
        eng.sync()
        e0, e1 = eng.event(), eng.event()
        times = {k: [] for k in forms}
        for _ in range(a.rounds):
            for k, f in forms.items():
                eng.record(e0)
                for _ in range(a.calls):
                    f()
                eng.record(e1)
                eng.sync()
                times[k].append(eng.elapsed_ms(e0, e1) / a.calls)
        be, bp, temps = bytes_moved(n, b, C, compact)
        print(f"{name}: n = {n}, int_bits {b}, C = {C}, {'compact uint32' if compact else '%d-limb' % limbs} operands; results equal"
              + (f"; {carried} of {n} elements differ from the element-wise sum" if carried >= 0 else ""), flush=True)
        for k, bts in (("elems", be), ("parent", bp)):
            t = times[k]
            med = statistics.median(t)
            print(f"  {k:6s}  {bts / 1e9:6.3f} GB moved{'' if k == 'elems' else ' (%.3f GB of temporaries)' % (temps / 1e9)}:  median {med:.4f} ms  "
                  f"min {min(t):.4f}  max {max(t):.4f}  spread {100 * (max(t) - min(t)) / med:.1f} %  -> {bts / med / 1e9:.2f} TB/s of its own bytes   "
                  f"windows: {' '.join('%.4f' % x for x in t)}", flush=True)
        me, mp = statistics.median(times["elems"]), statistics.median(times["parent"])
        print(f"  parent / elems = {mp / me:.2f}x (medians of {a.rounds} windows of {a.calls} calls)", flush=True)
        eng.close()


if __name__ == "__main__":
    main()
