"""Worker for the -m gpu test of flashe_amd.dist.SparseShardedRound at int_bits <= 64 with REAL kernels and several ranks on one GPU
(tests/test_gpu_sparse_small_width.py): HipOps exactly as production runs it, the exchange through tests/shm_comm.py instead of RCCL.
Every rank plays every client on the spans it owns (flashe_sparse_encrypt_aggregate_range_dev / flashe_sparse_decrypt_range_dev at
one limb); the gathered round trip must be the plain sparse sum, every rank's ciphertext entries the whole-list encrypt's.  No PyTorch."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from flashe_amd.dist import HipOps, SparseShardedRound  # noqa: E402
from flashe_amd.engine import Engine  # noqa: E402
from oracle import flashe_oracle as orc  # noqa: E402
from shm_comm import ShmComm, run_ranks  # noqa: E402

KEY = bytes(range(32))


def main(rank, world):
    comm = ShmComm(rank, world, os.environ["FLASHE_TEST_SHM_DIR"])
    orc.set_num_threads(2)
    eng = None
    for b, total, C, k, J in [(20, 300_007, 10, 3_000, 16), (20, 1_752 * 2 + 9, 4, 200, 1), (20, 999, 2, 999, 40), (20, 200_000, 70, 400, 16),
                              (64, 70_001, 3, 700, 16)]:
        L = 1
        eng = Engine(KEY, b, device=0)
        ops = HipOps(eng, None, comm)
        rng = [np.random.Generator(np.random.PCG64(470 + c)) for c in range(C)]
        ks = [k if c != 1 else max(k // 3, 1) for c in range(C)]
        locs = [np.sort(r.choice(total, kc, replace=False)).astype(np.uint32) for r, kc in zip(rng, ks)]
        vals = [r.integers(0, 2 ** 16, kc, dtype=np.uint64) for r, kc in zip(rng, ks)]
        zeros = [17 + c for c in range(C)]
        rnd = SparseShardedRound(ops, total, b, C, J, rank=rank, world=world)
        first, count = rnd.position_range()
        assert rnd.L == 1 and (count == 0 or first % ops.sparse_span() == 0) and first + count <= total
        rl, rp = [(ops.upload(l), 0) for l in locs], [(ops.upload(v), 0) for v in vals]
        rc = [(ops.alloc(max(kc, 1) * L), 0) for kc in ks]
        out = rnd.run(6, rl, ks, rp, 1, zeros, rc)
        want = np.full(total, np.uint64(sum(zeros)), dtype=np.uint64)
        for c in range(C):
            want[locs[c]] += vals[c] - np.uint64(zeros[c])
        want &= np.uint64((1 << b) - 1) if b < 64 else np.uint64(2 ** 64 - 1)
        got = ops.read((out, 0), total * L).reshape(total, L)
        assert np.array_equal(got[:, 0], want), (rank, b, total, C, "sparse position-sharded")
        for c in range(C):                              # this rank's ciphertext entries = the whole-list encrypt's, the others untouched
            full = orc.encrypt(KEY, 6, c, "single", J, b, vals[c])
            mine = (locs[c] >= first) & (locs[c] < first + count)
            have = ops.read(rc[c], ks[c] * L).reshape(ks[c], L)
            assert np.array_equal(have[mine], full[mine]) and not have[~mine].any(), (rank, b, c, "sparse ct entries")
    comm.barrier(eng)
    assert "torch" not in sys.modules
    if rank == 0:
        print("DIST_GPU_SPARSE_SMALL_OK")


if __name__ == "__main__":
    run_ranks(main)
