"""GPU: a sparse cohort's uploads in one chained launch from the floats (flashe_quantize_encrypt_sparse_cohort_dev,
prf_small_sparse_cohort_kernel<B>) against the two entry points it replaces and that other tests tie to the oracle --
flashe_quantize_cohort_dev into plaintexts, then flashe_encrypt_dev(SINGLE) per client -- compared as bytes: every upload element, every
trailing 'zzz' element, every zeros_dev[c]; and FlasheSparseCohort with front_end "fused" against the same cohort forced to "staged"."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEY = bytes(range(32))
WIDTHS = (16, 20, 23, 24, 32)
IT = 3
PATTERN = 0xA5
POISON = np.uint64(0xA5A5A5A5A5A5A5A5)
LAST_DRAW = float(np.nextafter(1.0, 0.0))            # 1 - 2^-53
EINVAL = -22

# K, n_jobs, clients, layer sizes: one block; empty chunks; every chunk ends in a partial block; whole tiles, rows that begin inside a
# half tile and inside a block, chunk ends
SHAPES = {
    "one": (1, 4, 1, (1,)),
    "empty-chunks": (13, 16, 128, (1, 5, 7)),
    "partial-blocks": (1000, 7, 3, (1, 383, 385, 231)),
    "tiles": (100_003, 16, 50, (1, 383, 385, 50_000, 7, 100_003 - 50_776)),
}
# storage dtype and flags of layer i (cycled): every source class, one LOOP_F64 row
STORAGE = ("float32", "float64", "float16", "bfloat16", "float32+loop64", "float32")


@pytest.fixture(scope="module")
def E():
    from flashe_amd import engine
    return engine


def _raw(x, storage):
    if storage == "float16":
        return x.astype(np.float16).view(np.uint16)
    if storage == "bfloat16":
        return (x.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    return x.astype(np.float64 if storage == "float64" else np.float32)


class _Cohort:
    """The arguments of both forms for C clients of one compact shape, the sources and draws in HBM."""

    def __init__(self, E, eng, K, sizes, C, norm=None, odd=0, seed=1):
        from flashe_amd import _lib
        code = {"float32": _lib.TENSOR_F32, "float64": _lib.TENSOR_F64, "float16": _lib.TENSOR_F16, "bfloat16": _lib.TENSOR_BF16}
        assert sum(sizes) == K
        g = np.random.Generator(np.random.PCG64(seed))
        self.K, self.C, self.stride = K, C, K + 1 + odd
        self.rows, at = [], 0
        kinds = []
        for i, size in enumerate(sizes):
            storage, _, loop = STORAGE[i % len(STORAGE)].partition("+")
            alpha = (0.37, 8.17121, 3e-3, 1.0, 1e-30, 0.1)[i % 6]
            flags, shift = (_lib.TENSOR_LOOP_F64 if loop else 0), 0.0
            if norm is not None and i % 2 == 1:
                flags |= _lib.TENSOR_SHIFT
                shift = -0.25 * alpha
                if norm == "wide" and storage != "float64":
                    flags |= _lib.TENSOR_SHIFT_WIDE
                    shift = -0.25 * alpha * (1 + 2.0 ** -40)
            self.rows.append((at, None, alpha, shift, _lib.TENSOR_F64 if storage == "float64" else _lib.TENSOR_F32, flags))
            kinds.append((storage, alpha, size))
            at += size
        self.keep, self.srcs, self.dts = [], [], []
        for c in range(C):
            srow, drow = [], []
            for storage, alpha, size in kinds:
                x = g.standard_normal(size) * alpha * 0.7
                x[:: max(1, size // 5)] = alpha                                    # clip edges
                x[1:: max(1, size // 3)] = -alpha * 1.5
                raw = _raw(x, storage)
                d = eng.alloc(raw.nbytes + 16)
                d.upload_at(0, raw)
                self.keep.append(d)
                srow.append(d.ptr)
                drow.append(code[storage])
            self.srcs.append(srow)
            self.dts.append(drow)
        u = g.random(C * self.stride)
        u[0], u[min(1, u.size - 1)] = 0.0, LAST_DRAW                               # (K = 1: the value's draw 0.0, its 'zzz' draw 1 - 2^-53)
        for c in range(C):
            u[c * self.stride + K] = (0.0, LAST_DRAW, 0.5)[c % 3] if c or K > 1 else LAST_DRAW
            if K > 2:
                u[c * self.stride + K - 1] = (LAST_DRAW, 0.0)[c % 2]
        self.du = eng.upload(u)
        self.zzz = [(0.0, 1.0, -1.0, 0.3, -7.0, 2.5)[c % 6] for c in range(C)]

    def uploads(self, E, eng, odd_client=None):
        """C upload vectors of K + 1 elements and one guard element each, poisoned; client `odd_client`'s at an address that is 8 mod 16."""
        bufs, views = [], []
        for c in range(self.C):
            nbytes = 8 * (self.K + 2)
            d = eng.alloc(nbytes + 16)
            eng.memset_dev(d, PATTERN, nbytes + 16)
            bufs.append(d)
            off = 8 if c == odd_client else 0
            assert (d.ptr + off) % 16 == off
            views.append(E.DeviceBufferView(d, off, nbytes))
        return bufs, views

    def staged(self, E, eng, b, idx, n_jobs, z64, eb=16):
        """The yardstick: quantize_cohort_dev, then encrypt_dev(SINGLE) per client -> (uploads [C, K + 2], zeros [C], plaintexts [C, K])."""
        K, C = self.K, self.C
        pts = [eng.alloc(8 * K + 16) for _ in range(C)]
        bufs, ups = self.uploads(E, eng)
        dz = eng.alloc(8 * C + 16)
        eng.quantize_cohort_dev(K, self.rows, self.srcs, self.dts, eb, self.du, self.stride, self.zzz, z64, pts, [u.ptr + 8 * K for u in ups], dz)
        for c in range(C):
            eng.encrypt_dev(IT, idx[c], E.SCHEME_SINGLE, K, n_jobs, pts[c], 1, ups[c])
        return (np.stack([u.download(np.uint64, K + 2) for u in ups]), dz.download(np.uint64, C),
                np.stack([p.download(np.uint64, K) for p in pts]))

    def fused(self, E, eng, idx, n_jobs, z64, eb=16, odd_client=None):
        bufs, ups = self.uploads(E, eng, odd_client)
        dz = eng.alloc(8 * self.C + 16)
        eng.memset_dev(dz, PATTERN, 8 * self.C + 16)
        ok = eng.quantize_encrypt_sparse_cohort_dev(IT, idx, self.K, n_jobs, self.rows, self.srcs, self.dts, eb, self.du, self.stride, self.zzz, z64, ups, dz)
        return ok, np.stack([u.download(np.uint64, self.K + 2) for u in ups]), dz.download(np.uint64, self.C)


def _same(got, want, *what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, bad[:6].tolist(), [hex(int(got[tuple(i)])) for i in bad[:3]], [hex(int(want[tuple(i)])) for i in bad[:3]], len(bad))


def _case(E, b, shape, norm=None, idx0=5, idx=None, z64=None, odd_client=None, odd=0):
    K, n_jobs, C, sizes = SHAPES[shape] if isinstance(shape, str) else shape
    z64 = (b % 2 == 0) if z64 is None else z64
    idx = list(range(idx0, idx0 + C)) if idx is None else idx
    odd_client = None if odd_client is None else min(odd_client, C - 1)
    eng = E.Engine(KEY, b, device=0)
    co = _Cohort(E, eng, K, sizes, C, norm=norm, odd=odd, seed=b + K)
    want_up, want_z, pts = co.staged(E, eng, b, idx, n_jobs, z64)
    ok, got_up, got_z = co.fused(E, eng, idx, n_jobs, z64, odd_client=odd_client)
    assert ok, "the chained sparse cohort launch declined the shape"
    assert (want_up[:, K + 1] == POISON).all() and (got_up[:, K + 1] == POISON).all(), "a write behind element K"
    _same(got_up[:, :K], want_up[:, :K], "ciphertexts", b, shape)
    _same(got_up[:, K], want_up[:, K], "tail", b, shape)
    _same(got_z, want_z, "zeros", b, shape)
    assert (got_up[:, K] == got_z).all()
    assert (got_up[:, :K] < (np.uint64(1) << np.uint64(b))).all()
    eng.close()
    return idx, n_jobs, pts, got_up


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("b", WIDTHS)
def test_fused_equals_quantise_then_encrypt(E, oracle, b, shape):
    """All five widths x the four shapes (C = 1, 128, 3, 50; cipher indices from 5, iter 3, n_jobs given); client 1's upload 8 but not
    16-byte aligned.  The first two shapes also against tests/oracle_ops.py on the yardstick's plaintexts."""
    from oracle_ops import HostBuf, OracleOps
    idx, n_jobs, pts, got = _case(E, b, shape, odd_client=1)
    if shape in ("one", "empty-chunks"):
        K, C = pts.shape[1], pts.shape[0]
        ops = OracleOps(b)
        src, dst = [HostBuf(K) for _ in range(C)], [HostBuf(K) for _ in range(C)]
        for c in range(C):
            src[c].a[:K] = pts[c]
        ops.encrypt_batch(IT, idx, E.SCHEME_SINGLE, K, n_jobs, [(s, 0) for s in src], 1, [(d, 0) for d in dst])
        for c in range(C):
            assert np.array_equal(got[c, :K], dst[c].a[:K]), (b, shape, c)


@pytest.mark.parametrize("norm,b", [("shift", 20), ("wide", 23)])
def test_normalised_rows_go_through_the_stage_pass(E, norm, b):
    _case(E, b, "tiles", norm=norm, odd_client=0)


def test_non_consecutive_indices_and_odd_draw_stride(E):
    K, n_jobs, _C, sizes = SHAPES["partial-blocks"]
    _case(E, 20, (K, n_jobs, 5, sizes), idx=[5, 9, 6, 4_000_000_000, 0], odd=1)


def test_a_chain_that_is_not_cut(E):
    """Enough tiles for every wave of the chip: one chain of two links over the whole vector."""
    K = 304 * 16 * 128 * 6 + 77
    _case(E, 20, (K, 16, 2, (1, 1023, K - 1024)), odd_client=1)


def _refused(E, eng, K=13, C=2, n=None, stride=None):
    """One call that the library must decline: returns what the binding returned; every output still holds its pattern."""
    co = _Cohort(E, eng, max(K, 1), (max(K, 1),), C)
    if K == 0:
        co.K = 0
    bufs, ups = co.uploads(E, eng)
    dz = eng.alloc(8 * C + 16)
    eng.memset_dev(dz, PATTERN, 8 * C + 16)
    rc = eng.quantize_encrypt_sparse_cohort_dev(IT, list(range(5, 5 + C)), co.K if n is None else n, 16, co.rows, co.srcs, co.dts, min(16, eng.int_bits), co.du,
                                                co.stride if stride is None else stride, co.zzz, True, ups, dz)
    eng.sync()
    for d in bufs:
        assert (d.download(np.uint64, d.nbytes // 8) == POISON).all(), "a refused call wrote an upload"
    assert (dz.download(np.uint64, C) == POISON).all(), "a refused call wrote zeros_dev"
    return rc


@pytest.mark.parametrize("b", [40, 64, 128, 8, 17])
def test_other_widths_are_refused(E, b):
    eng = E.Engine(KEY, b, device=0)
    assert _refused(E, eng) is False


def test_refusals_launch_nothing(E, monkeypatch):
    eng = E.Engine(KEY, 20, device=0)
    assert _refused(E, eng, C=129) is False
    assert _refused(E, eng, n=1 << 32, stride=(1 << 32) + 1) is False
    assert _refused(E, eng, K=0) is False
    monkeypatch.setenv("FLASHE_CHAIN", "0")
    off = E.Engine(KEY, 20, device=0)
    assert _refused(E, off) is False
    monkeypatch.delenv("FLASHE_CHAIN")
    # bad arguments: FLASHE_EINVAL, as flashe_quantize_cohort_dev
    co = _Cohort(E, eng, 13, (13,), 2)
    bufs, ups = co.uploads(E, eng)
    dz = eng.alloc(32)
    for bad in ({"stride": 13}, {"eb": 21}, {"eb": 0}, {"alpha": -1.0}, {"dtype": 77}, {"null": True}):
        rows = [co.rows[0][:2] + (bad.get("alpha", co.rows[0][2]),) + co.rows[0][3:]]
        dts = [[bad.get("dtype", d) for d in row] for row in co.dts]
        with pytest.raises(E.FlasheError) as err:
            eng.quantize_encrypt_sparse_cohort_dev(IT, [5, 6], 13, 16, rows, co.srcs, dts, bad.get("eb", 16), co.du, bad.get("stride", co.stride), co.zzz, True,
                                                   [None, ups[1]] if bad.get("null") else ups, dz)
        assert err.value.code == EINVAL, bad
    with pytest.raises(E.FlasheError):
        eng.quantize_cohort_dev(13, co.rows, co.srcs, co.dts, 16, co.du, 13, co.zzz, True, ups, None, dz)


def test_another_prf_backend_is_refused(E, monkeypatch):
    """The bit-sliced PRF lives in the build's second library: a ctx of it with FLASHE_PRF_BACKEND=bitslice declines."""
    from flashe_amd import _lib
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), "libflashe_hip_bitslice.so")
    assert os.path.exists(path), "build() makes the bit-sliced library next to the product library"
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", path)
    monkeypatch.setenv("FLASHE_PRF_BACKEND", "bitslice")
    eng = E.Engine(KEY, 20, device=0)
    try:
        assert _refused(E, eng) is False
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ through FlasheSparseCohort
def _args(b):
    return {"quantize": {"int_bits": b, "batch": False, "element_bits": 16, "padding": True, "secure": True},
            "precompute": {"enable": False, "num_params": 11}, "mask": "dynamic"}


try:
    # (asked at collection: once a test has created an engine, the framework of the same process no longer finds its device)
    import torch as _torch_mod
    _TORCH_GPU = _torch_mod.cuda.is_available()
except ImportError:
    _TORCH_GPU = False


def _models(C, sizes, seed, torch=None):
    """C models; layer 1 of 3 is float64; with torch every even layer is a device tensor, the others stay host arrays."""
    g = np.random.Generator(np.random.PCG64(seed))
    out = []
    for c in range(C):
        m = {}
        for i, s in enumerate(sizes):
            x = (g.standard_normal(s) * 0.05 + 0.01 * c).astype(np.float64 if i % 3 == 1 else np.float32).reshape((s,) if i % 2 else (1, s))
            m[f"l{i:02d}"] = torch.from_numpy(x).cuda() if torch is not None and i % 2 == 0 else x
        out.append(m)
    return out


def _hexes(vals):
    return [float(v).hex() for v in vals]


def _cohort_rounds(b, prefer, sorted_lists, C=3, rounds=3, spy=None, torch=None):
    """-> per round (front_end, uploads, aggregate, floats, mean / std hex, generator state, alphas, shape_dict).  sorted_lists: the
    whole round from dense models (sparsify's own strictly increasing lists); otherwise compact layers and the arbiter's lists given
    directly, client 1's list in descending order: the unsorted branch."""
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheSparseCohort
    cm.N_JOBS = 16
    sizes = [1, 1013, 256 * 9 + 17, 30_011]
    names, total = [f"l{i:02d}" for i in range(len(sizes))], sum(sizes)
    shapes = {f"l{i:02d}": ((s,) if i % 2 else (1, s)) for i, s in enumerate(sizes)}
    ks = [max(1, int(np.floor(0.1 * s))) for s in sizes]
    co = FlasheSparseCohort(_args(b), first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, sparsity=0.1)
    co.prefer_front_end = prefer
    if spy is not None:
        spy(co)
    out = []
    for it in range(1, rounds + 1):
        co.set_iter_index(it)
        if sorted_lists:
            co.sparsify(_models(C, sizes, 300 + it, torch), names)
            assert co.dynamic_masking() == "single"
            np.random.seed(4000 + it)
            up = co.quantize_encrypt(normalize=True)
        else:
            g = np.random.Generator(np.random.PCG64(900 + it))
            lists = [np.sort(g.choice(total, sum(ks), replace=False)) for _ in range(C)]
            lists[1 % C] = lists[1 % C][::-1].copy()
            assert co.dynamic_masking("single", [l.tolist() for l in lists], total) == "single"
            compact = [{nm: (g.standard_normal(k) * 0.05).astype(np.float64 if i % 3 == 1 else np.float32) for i, (nm, k) in enumerate(zip(names, ks))}
                       for _ in range(C)]
            co.shape_dict_used_for_sparsification = dict(shapes)
            np.random.seed(4000 + it)
            up = co.quantize_encrypt(compact=compact, normalize=True)
            assert not co._sorted
        assert up.path == "sparse-cohort"
        back = co.decrypt_unquantize(unnormalize=True)
        out.append((up.front_end, [u.to_host().tobytes() for u in up.uploads], up.aggregate.to_host().tobytes(),
                    [np.asarray(back._weights[k]).tobytes() for k in names], _hexes(co.quantizer.past_layer_mean_list),
                    _hexes(co.quantizer.past_layer_std_list), np.random.get_state()[1].tobytes(), np.random.get_state()[2],
                    _hexes(co.alpha_list), dict(co.shape_dict)))
    return out


@pytest.mark.parametrize("sorted_lists", [True, False])
def test_cohort_fused_equals_staged(sorted_lists):
    calls = []

    def spy(co):
        eng = co.engine
        real = eng.quantize_cohort_dev
        eng.quantize_cohort_dev = lambda *a, **k: (calls.append("quantize_cohort_dev"), real(*a, **k))[1]

    fused = _cohort_rounds(20, None, sorted_lists, spy=spy)
    assert calls == [], "the fused form allocates and writes no plaintexts"
    staged = _cohort_rounds(20, "staged", sorted_lists, spy=spy)
    assert len(calls) == 3
    assert [r[0] for r in fused] == ["fused"] * 3 and [r[0] for r in staged] == ["staged"] * 3
    for it, (f, s) in enumerate(zip(fused, staged)):
        for part, (a, b) in enumerate(zip(f[1:], s[1:])):
            assert a == b, (it, part)


def test_cohort_fused_equals_staged_with_tensors():
    torch = pytest.importorskip("torch")
    if not (_TORCH_GPU and torch.cuda.is_available()):
        pytest.skip("no GPU visible to torch")
    fused = _cohort_rounds(20, None, True, torch=torch)
    staged = _cohort_rounds(20, "staged", True, torch=torch)
    assert [r[0] for r in fused] == ["fused"] * 3 and [r[0] for r in staged] == ["staged"] * 3
    for it, (f, s) in enumerate(zip(fused, staged)):
        for part, (a, b) in enumerate(zip(f[1:], s[1:])):
            assert a == b, (it, part)


@pytest.mark.parametrize("b", [128, 40])
def test_other_widths_stay_staged(b):
    assert [r[0] for r in _cohort_rounds(b, None, True, rounds=1)] == ["staged"]


def test_library_calls_do_not_grow_with_the_cohort():
    """The engine methods quantize_encrypt calls, counted: the same for 2 and for 9 clients."""
    from flashe_amd import engine as E

    def count(C):
        seen = []

        def spy(co):
            eng = co.engine
            for name in dir(E.Engine):
                if name.endswith("_dev") and callable(getattr(eng, name)):
                    real = getattr(eng, name)
                    setattr(eng, name, lambda *a, _r=real, _n=name, **k: (seen.append(_n), _r(*a, **k))[1])
            self_q = co.quantize_encrypt

            def traced(*a, **k):
                seen.append("<quantize_encrypt>")
                try:
                    return self_q(*a, **k)
                finally:
                    seen.append("</quantize_encrypt>")
            co.quantize_encrypt = traced

        _cohort_rounds(20, None, True, C=C, rounds=1, spy=spy)
        a, z = seen.index("<quantize_encrypt>"), seen.index("</quantize_encrypt>")
        return seen[a + 1:z]

    two, nine = count(2), count(9)
    assert "quantize_encrypt_sparse_cohort_dev" in two and "encrypt_dev" not in two and "quantize_cohort_dev" not in two
    assert two == nine, (two, nine)
