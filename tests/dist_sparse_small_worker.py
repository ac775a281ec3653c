"""Worker for tests/test_sparse_small_width_host.py: flashe_amd.dist.SparseShardedRound at int_bits <= 64 over gloo, world_size ranks
on CPU.  The ranks' position ranges, the gathered round trip (the plain sparse sum) and every rank's ciphertext entries (those of the
whole-list encrypt) are checked; local arithmetic is the oracle-backed ops double."""
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from flashe_amd.dist import SparseShardedRound  # noqa: E402
from oracle import flashe_oracle as orc  # noqa: E402
from oracle_ops import GlooComm, OracleOps  # noqa: E402

KEY = bytes(range(32))


def main():
    dist.init_process_group("gloo")
    comm = GlooComm()
    rank, world = comm.rank, comm.world
    orc.set_num_threads(1)
    for b, total, C, k, n_jobs in [(20, 20_000, 5, 700, 16), (20, 1_752 * 2 + 5, 3, 60, 1), (64, 900, 4, 900, 40), (20, 1_752 * world, 2, 100, 16)]:
        ops = OracleOps(b, comm)
        rnd = SparseShardedRound(ops, total, b, C, n_jobs, rank=rank, world=world)
        first, count = rnd.position_range()
        assert (count == 0 or first % ops.sparse_span() == 0) and first + count <= total
        assert first == min(total, rank * rnd.slice) and first + count == min(total, (rank + 1) * rnd.slice) and world * rnd.slice >= total
        rng = [np.random.Generator(np.random.PCG64(530 + c)) for c in range(C)]
        ks = [k if c != 1 else max(k // 3, 1) for c in range(C)]
        locs = [np.sort(r.choice(total, kc, replace=False)).astype(np.uint32) for r, kc in zip(rng, ks)]
        vals = [r.integers(0, 2 ** 16, kc, dtype=np.uint64) for r, kc in zip(rng, ks)]
        zeros = [11 + c for c in range(C)]
        rl, rp = [(ops.upload(l), 0) for l in locs], [(ops.upload(v), 0) for v in vals]
        rc = [(ops.alloc(max(kc, 1)), 0) for kc in ks]
        out = rnd.run(9, rl, ks, rp, 1, zeros, rc)
        want = np.full(total, np.uint64(sum(zeros)), dtype=np.uint64)
        for c in range(C):
            want[locs[c]] += vals[c] - np.uint64(zeros[c])
        want &= np.uint64((1 << b) - 1) if b < 64 else np.uint64(2 ** 64 - 1)
        res = ops.read((out, 0), total).reshape(total)
        assert np.array_equal(res, want), (rank, b, total, C, "gathered")
        for c in range(C):
            full = orc.encrypt(KEY, 9, c, "single", n_jobs, b, vals[c])
            mine = (locs[c] >= first) & (locs[c] < first + count)
            got = ops.read(rc[c], ks[c]).reshape(ks[c], 1)
            assert np.array_equal(got[mine], full[mine]) and not got[~mine].any(), (rank, c, "ciphertext entries")
    dist.barrier()
    if rank == 0:
        print("DIST_SPARSE_SMALL_OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
