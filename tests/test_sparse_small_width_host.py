"""CPU tests of the sparse round at int_bits <= 64 sharded by position ranges (flashe_amd.dist.SparseShardedRound, which raised
ValueError below 65 bits) and of the budget of its kernel, span_prf_small_kernel (stream.hip), per the code objects inside the built
library (tools/kernel_resources.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

KEY = bytes(range(32))


@pytest.mark.parametrize("b,J", [(20, 16), (20, 1), (64, 40), (7, 16)])
def test_single_rank_sparse_position_sharding_one_limb(oracle, b, J):
    """SparseShardedRound(OracleOps(b)) on one rank: the position range is the whole vector, the round trip is the plain sparse sum
    (mod 2^b), the ciphertexts are the oracle's single-mask encrypts of the compact uploads."""
    from flashe_amd.dist import SparseShardedRound
    from oracle_ops import OracleOps
    total, C, k = 7_000, 4, 250
    ops = OracleOps(b)
    rnd = SparseShardedRound(ops, total, b, C, J)
    assert rnd.position_range() == (0, total) and rnd.L == 1
    rng = [np.random.Generator(np.random.PCG64(910 + c)) for c in range(C)]
    locs = [np.sort(r.choice(total, k, replace=False)).astype(np.uint32) for r in rng]
    vals = [r.integers(0, 2 ** min(b - 2, 60), k, dtype=np.uint64) for r in rng]
    rl, rp = [(ops.upload(l), 0) for l in locs], [(ops.upload(v), 0) for v in vals]
    rc = [(ops.alloc(k), 0) for _ in range(C)]
    out = rnd.run(2, rl, [k] * C, rp, 1, [5] * C, rc)
    want = np.full(total, np.uint64(5 * C), dtype=np.uint64)
    for c in range(C):
        want[locs[c]] += vals[c] - np.uint64(5)
    want &= np.uint64((1 << b) - 1) if b < 64 else np.uint64(2 ** 64 - 1)
    assert np.array_equal(ops.read((out, 0), total).reshape(total), want)
    for c in range(C):
        assert np.array_equal(ops.read(rc[c], k).reshape(k, 1), oracle.encrypt(KEY, 2, c, "single", J, b, vals[c]))


@pytest.mark.parametrize("world,port", [(2, 29561), (3, 29562)])
def test_sparse_position_sharding_one_limb_gloo(world, port, oracle):
    """The same round at int_bits 20 and 64 over gloo with world 2 and 3 (tests/dist_sparse_small_worker.py)."""
    env = dict(os.environ, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "dist_sparse_small_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "DIST_SPARSE_SMALL_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_span_prf_small_kernel_budget():
    """Every instantiation of span_prf_small_kernel: no scratch, at most 128 VGPRs (four 1,024-thread waves per SIMD), one workgroup
    of 1,024 lanes, and its static LDS (AES tables + one u64 accumulator plane of a span) within the CU's 160 KiB."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.resources(os.path.join(ROOT, "flashe_amd", "libflashe_hip.so"))
    sp = {k: r for k, r in res.items() if "span_prf_small_kernel<" in k}
    assert len(sp) == 4, list(sp)
    for k, r in sp.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, (k, r)
        assert r["vgpr"] + r["agpr"] <= 128, (k, r)
        assert r["max_workgroup"] == 1024, (k, r)
        assert r["lds_bytes_static"] <= 160 * 1024, (k, r)
