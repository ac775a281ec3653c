"""bench.py --dump-outputs: what the last timed step computed, written as float64 .npy files (exact, bounded, the same from run to run)."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

KEY = bytes(range(32))


@pytest.fixture
def bench_mod():
    saved = dict(os.environ)            # (bench.py fills in a few runtime variables at import)
    try:
        yield importlib.import_module("bench")
    finally:
        os.environ.clear()
        os.environ.update(saved)


def limbs(a):
    """float64 columns (low, high 32 bits per limb) -> uint64 limbs."""
    a = a.astype(np.uint64)
    return a[:, 0::2] | (a[:, 1::2] << np.uint64(32))


def test_dump_outputs_is_exact_and_bounded(bench_mod, tmp_path):
    rng = np.random.Generator(np.random.PCG64(5))
    big = rng.integers(0, 2 ** 64, (3_000_001, 2), dtype=np.uint64)
    small = rng.integers(0, 2 ** 64, 1000, dtype=np.uint64)
    u32 = rng.integers(0, 2 ** 32, 777, dtype=np.uint32)
    f64 = rng.standard_normal(500)
    outs = {"big": lambda: big, "small": lambda: small, "u32": lambda: u32, "f64": lambda: f64}
    outs.update({f"more_{i}": (lambda: big) for i in range(8)})
    for d in ("a", "b"):
        bench_mod.dump_outputs(str(tmp_path / d), outs)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench_mod.DUMP_BUDGET_BYTES
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float64 and np.array_equal(a, b), f
    got, rows = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "a" / "big_rows.npy").astype(np.int64)
    assert 0 < len(rows) < len(big) and np.all(np.diff(rows) > 0) and np.array_equal(limbs(got), big[rows])
    assert np.array_equal(limbs(np.load(tmp_path / "a" / "small.npy"))[:, 0], small) and not os.path.exists(tmp_path / "a" / "small_rows.npy")
    assert np.array_equal(np.load(tmp_path / "a" / "u32.npy")[:, 0], u32.astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "a" / "f64.npy")[:, 0], f64)


@pytest.mark.gpu
def test_bench_dump_outputs_of_the_timed_round(bench_mod, oracle, tmp_path):
    """The default round at reduced size, twice with the same arguments: the files are identical, the decrypted sum is the plaintext
    sum and a ciphertext is the oracle's encrypt at the last timed step's iteration (step k of the timed region runs iteration k)."""
    n, K, J, b = 300_007, 3, 16, 128
    lines = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(K), "--warmup", "1", "--settle-rounds", "2",
                            "--n", str(n), "--no-cpu-baseline", "--no-e2e", "--no-unchained", "--dump-outputs", str(tmp_path / d)],
                           capture_output=True, text=True, timeout=600, env=dict(os.environ, OMP_WAIT_POLICY="passive"))
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith('{"metric"')][0]))
    assert all(d["steps"] == K and d["ms_per_step"] > 0 for d in lines)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b")) and "decrypted_sum.npy" in files and "ciphertext_c9.npy" in files
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench_mod.DUMP_BUDGET_BYTES
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f

    def load(name):
        rows = tmp_path / "a" / f"{name}_rows.npy"
        return limbs(np.load(tmp_path / "a" / f"{name}.npy")), (np.load(rows).astype(np.int64) if rows.exists() else np.arange(n))

    pts = [bench_mod.plaintext(c, n, b) for c in range(10)]
    got, rows = load("decrypted_sum")
    lo, hi = bench_mod.sum_mod(pts, n, b)
    assert np.array_equal(got[:, 0], lo[rows]) and np.array_equal(got[:, 1], hi[rows])
    got, rows = load("ciphertext_c3")
    assert np.array_equal(got, oracle.encrypt(KEY, K - 1, 3, "double", J, b, pts[3])[rows])
