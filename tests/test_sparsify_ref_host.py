"""The sparsifier's NumPy reference (tests/sparsify_ref.py) against itself, the C oracle and the reference project's golden rounds, on
every builder of edge inputs that the GPU test (tests/test_gpu_sparsify_edges.py) feeds the kernels.  No GPU."""
import numpy as np
import pytest

from conftest import load_golden
import sparsify_ref as sr


def _same(a, b):
    return all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _cases(kind):
    for bi, build in enumerate(sr.BUILDERS):
        for n in sr.SIZES:
            layer, res, ks = build(kind, n, 1000 * bi + n)
            assert {0, 1, n // 2, n - 1, n} & set(range(n + 1)) <= set(ks)
            yield build.__name__, layer, res, ks


@pytest.mark.parametrize("kind", sr.KINDS)
def test_references_agree_on_every_builder(oracle, kind):
    """Stable argsort == key-bits lexsort == the C oracle, byte for byte on loc, vals and the new residual, with a residual and without."""
    count = 0
    for name, layer, res, ks in _cases(kind):
        x = sr.widen(layer)
        for k in ks:
            for r in (res, None):
                a = sr.topk_ref(layer, k, r)
                b = sr.topk_ref(layer, k, r, rank=sr.rank_keybits)
                c = oracle.sparsify(x, k, np.zeros_like(x) if r is None else r)
                assert a[0].dtype == np.uint32 and a[1].dtype == a[2].dtype == x.dtype and len(a[0]) == len(a[1]) == k
                assert _same(a, b) and _same(a, c), (kind, name, layer.size, k, r is None)
                assert np.all(np.diff(a[0].astype(np.int64)) > 0)
                count += 1
    assert count >= 2 * 5 * len(sr.BUILDERS) * (len(sr.SIZES) - 3)          # (nothing filtered away: sizes 1, 3 and 4 have fewer distinct k)


def test_references_reproduce_the_golden_rounds():
    for c in load_golden("sparsify.json")["cases"]:
        dt = np.dtype(c["dtype"])
        for rank in (sr.rank_stable, sr.rank_keybits):
            remain = np.zeros(c["n"], dtype=dt)
            for rd in c["rounds"]:
                layer = np.frombuffer(bytes.fromhex(rd["layer"]), dtype=dt)
                loc, vals, remain = sr.topk_ref(layer, rd["k"], remain, rank=rank)
                assert [int(v) for v in loc] == rd["location"]
                assert vals.tobytes().hex() == rd["masked"] and remain.tobytes().hex() == rd["remain"]


@pytest.mark.parametrize("mutate,rank", [("ties_low", sr.rank_stable), ("after_residual", sr.rank_stable), ("keep_sign", sr.rank_keybits)])
def test_the_inputs_tell_a_bent_rule_from_the_right_one(mutate, rank):
    """Ties to the lower index, ranking after the residual is added, a key that keeps the sign bit: each bent reference must differ from
    the right one on at least one builder, for every kind -- the inputs discriminate."""
    for kind in sr.KINDS:
        caught = set()
        for name, layer, res, ks in _cases(kind):
            if any(not _same(sr.topk_ref(layer, k, res), sr.topk_ref(layer, k, res, rank=rank, mutate=mutate)) for k in ks):
                caught.add(name)
        assert caught, (kind, mutate)


def test_widen_is_exact():
    h = np.arange(0, 0x7c01, dtype=np.uint16)                                  # every non-negative finite float16 and inf
    w = sr.widen(h.view(np.float16))
    assert w.dtype == np.float32 and np.array_equal(w.astype(np.float16).view(np.uint16), h)
    b = np.array([0x0000, 0x0001, 0x007f, 0x0080, 0x3f80, 0x7f7f, 0x7f80, 0x8001, 0xff80], dtype=np.uint16)
    assert [int(v) for v in sr.widen(b).view(np.uint32)] == [int(v) << 16 for v in b]


def test_packed_ref_is_to_big_int(oracle):
    """packed_ref == the integer `_to_bytes` builds (jzf_weights.py:36-84: shift left, add the next -- the first entry most significant)
    == the oracle's pack, the host twin of what weights.to_big_int runs on the device (the GPU test compares with to_big_int itself);
    K bits a multiple of 64 and not, K = 1."""
    rng = np.random.Generator(np.random.PCG64(3))
    for bits in (1, 5, 12, 13, 16, 31, 32):
        for K in (1, 2, 3, 4, 63, 64, 65, 1000):
            loc = rng.integers(0, 1 << bits, K, dtype=np.uint64)
            limbs = sr.packed_ref(loc.astype(np.uint32), bits)
            want = 0
            for v in loc:
                want = (want << bits) + int(v)
            assert limbs.size == (K * bits + 63) // 64 and int.from_bytes(limbs.tobytes(), "little") == want
            assert np.array_equal(limbs, oracle.pack(loc, bits)), (bits, K)
