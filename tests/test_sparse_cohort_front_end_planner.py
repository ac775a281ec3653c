"""CPU: plan_sparse_cohort's front_end -- which sparse cohorts take the chained quantise + encrypt launch
(flashe_quantize_encrypt_sparse_cohort_dev), decided without a device -- and FlasheSparseCohort's fallback: on an oracle-backed engine double
(tests/fake_engine.py, extended here with a flat memory model and the sparse cohort's entry points) a cohort whose engine lacks the new
method, or whose library declines (False), runs the staged form with identical results."""
import numpy as np
import pytest

import codec_ref as R
from fake_engine import OracleEngine
from oracle import flashe_oracle as orc

KEY = bytes(range(32))


def _models(C, dtypes=("float32",), sizes=(40, 7, 300)):
    g = np.random.Generator(np.random.PCG64(5))
    return [{f"l{i}": (g.standard_normal(s) * 0.05).astype(dtypes[i % len(dtypes)]) for i, s in enumerate(sizes)} for _ in range(C)]


# ------------------------------------------------------------------------------------------------ the planner
@pytest.mark.parametrize("b", [16, 20, 23, 24, 32])
def test_the_five_widths_are_fused(b):
    from flashe_amd.block import plan_sparse_cohort
    p = plan_sparse_cohort(_models(3), 0.1, b)
    assert (p.path, p.front_end, p.front_end_reason) == ("sparse-cohort", "fused", "")
    assert p.K == 4 + 1 + 30 and p.n_elems == p.K + 1


@pytest.mark.parametrize("b", [40, 64, 128, 8, 17, 31])
def test_other_widths_are_staged(b):
    from flashe_amd.block import plan_sparse_cohort
    p = plan_sparse_cohort(_models(3), 0.1, b)
    assert (p.path, p.front_end) == ("sparse-cohort", "staged")
    assert f"int_bits {b}" in p.front_end_reason


def test_128_clients_are_fused_129_are_not():
    from flashe_amd.block import plan_sparse_cohort
    m = _models(1)
    assert plan_sparse_cohort(m * 128, 0.1, 20).front_end == "fused"
    p = plan_sparse_cohort(m * 129, 0.1, 20)
    assert (p.path, p.front_end) == ("sparse-cohort", "staged") and "129 clients" in p.front_end_reason


@pytest.mark.parametrize("kw,why", [({"choice": "double"}, "masking choice"), ({"batch": True}, "batched"), ({"precompute": True}, "precomputed"),
                                    ({"fuse": False}, "fuse is off")])
def test_the_per_client_path_is_staged_for_its_own_reason(kw, why):
    from flashe_amd.block import plan_sparse_cohort
    p = plan_sparse_cohort(_models(3), 0.1, 20, **kw)
    assert (p.path, p.front_end) == ("per-client", "staged")
    assert why in p.reason and p.front_end_reason == p.reason


def test_a_layer_that_is_float64_for_some_clients_only_is_staged():
    from flashe_amd.block import plan_sparse_cohort
    ms = _models(3)
    ms[1]["l1"] = ms[1]["l1"].astype(np.float64)
    p = plan_sparse_cohort(ms, 0.1, 20)
    assert (p.path, p.front_end) == ("per-client", "staged") and "float64" in p.front_end_reason
    # float64 for every client is one compute class: fused
    assert plan_sparse_cohort(_models(3, ("float32", "float64")), 0.1, 20).front_end == "fused"


def test_flashe_chain_0_is_staged(monkeypatch):
    from flashe_amd.block import plan_sparse_cohort
    monkeypatch.setenv("FLASHE_CHAIN", "0")
    p = plan_sparse_cohort(_models(3), 0.1, 20)
    assert (p.path, p.front_end, p.front_end_reason) == ("sparse-cohort", "staged", "FLASHE_CHAIN=0")
    monkeypatch.setenv("FLASHE_CHAIN", "1")
    assert plan_sparse_cohort(_models(3), 0.1, 20).front_end == "fused"


# ------------------------------------------------------------------------------------------------ the cohort on an engine double
class _Buf:
    """A block of the double's flat address space."""

    def __init__(self, engine, nbytes):
        self.engine, self.nbytes = engine, int(nbytes)
        self.ptr = engine._next
        engine._next += (self.nbytes + 255) & ~255
        self.mem = np.zeros(self.nbytes, dtype=np.uint8)
        engine._blocks[self.ptr] = self

    def upload(self, arr):
        return self.upload_at(0, arr)

    def upload_at(self, off, arr):
        raw = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        assert off + raw.size <= self.nbytes
        self.mem[off:off + raw.size] = raw
        return self

    def download(self, dtype=np.uint64, count=None):
        return self.download_at(0, dtype, self.nbytes // np.dtype(dtype).itemsize if count is None else count)

    def download_at(self, off, dtype, count):
        return self.mem[off:off + count * np.dtype(dtype).itemsize].view(dtype).copy()

    def free(self):
        pass


class _Bounds:
    def __init__(self, log):
        self.log = log

    def recompute(self, locs, ks, keep=None):
        self.log.append("span_bounds.recompute")
        return self


class SparseEngine(OracleEngine):
    """OracleEngine + what FlasheSparseCohort.quantize_encrypt calls, on host memory with device-style addresses.  No chained launch."""

    def __init__(self, key, int_bits, device=0, stream=None):
        super().__init__(key, int_bits, device, stream)
        self._next, self._blocks, self.log = 1 << 20, {}, []

    def alloc(self, nbytes):
        return _Buf(self, nbytes)

    def alloc_vec(self, n, limbs=None):
        return _Buf(self, max(8 * n * (limbs or self.limbs), 16))

    def upload(self, arr):
        a = np.ascontiguousarray(arr)
        return _Buf(self, max(a.nbytes, 16)).upload(a)

    def hold(self, keep):
        pass

    def _at(self, ref, nbytes):
        """nbytes at a block, a vector or a raw address."""
        ptr = ref if isinstance(ref, int) else ref.ptr
        base = max(b for b in self._blocks if b <= ptr)
        blk = self._blocks[base]
        assert ptr - base + nbytes <= blk.nbytes, "an access beyond the block"
        return blk.mem[ptr - base:ptr - base + nbytes]

    def _quantize(self, n, layers, srcs, dtypes, element_bits, u, u_stride, zzz, zzz_is_f64):
        """-> (plaintexts [C, n], zeros [C]): stage_layers_kernel's normalise rule and the reference codec, per client and row."""
        from flashe_amd import _lib
        dt_of = {_lib.TENSOR_F32: np.float32, _lib.TENSOR_F64: np.float64}
        C = len(srcs)
        draws = self._at(u, 8 * ((C - 1) * u_stride + n + 1)).view(np.float64)
        pts, zeros = np.zeros((C, n), dtype=np.uint64), np.zeros(C, dtype=np.uint64)
        ends = [row[0] for row in layers[1:]] + [n]
        for c in range(C):
            for li, ((start, _p, alpha, shift, _dt, flags), end) in enumerate(zip(layers, ends)):
                x = self._at(srcs[c][li], (end - start) * np.dtype(dt_of[dtypes[c][li]]).itemsize).view(dt_of[dtypes[c][li]]).copy()
                if flags & _lib.TENSOR_SHIFT:
                    x = R.ref_shift(x, np.float64(shift) if flags & _lib.TENSOR_SHIFT_WIDE else float(shift))
                if flags & _lib.TENSOR_LOOP_F64:
                    x = x.astype(np.float64)
                pts[c, start:end] = R.ref_quantize(x, alpha, element_bits, draws[c * u_stride + start:c * u_stride + end]).astype(np.uint64)
            z = np.array([zzz[c]], dtype=np.float64 if zzz_is_f64 else np.float32)
            zeros[c] = R.ref_quantize(z, 1.0, element_bits, draws[c * u_stride + n:c * u_stride + n + 1])[0]
        return pts, zeros

    def quantize_cohort_dev(self, n, layers, srcs, dtypes, element_bits, u, u_stride, zzz, zzz_is_f64, pts, tails, zeros):
        self.log.append("quantize_cohort_dev")
        p, z = self._quantize(n, layers, srcs, dtypes, element_bits, u, u_stride, zzz, zzz_is_f64)
        for c in range(len(srcs)):
            self._at(pts[c], 8 * n)[:] = p[c].view(np.uint8)
            if tails is not None and tails[c]:
                self._at(tails[c], 8 * self.limbs)[:] = 0
                self._at(tails[c], 8)[:] = z[c:c + 1].view(np.uint8)
        self._at(zeros, 8 * len(srcs))[:] = z.view(np.uint8)

    def encrypt_dev(self, it, idx, scheme, n, n_jobs, pt, pt_limbs, ct):
        self.log.append("encrypt_dev")
        src = self._at(pt, 8 * n * pt_limbs).view(np.uint64).reshape(n, pt_limbs)
        out = orc.encrypt(self.key, it, idx, self._sch(scheme), n_jobs, self.int_bits, np.ascontiguousarray(src))
        self._at(ct, 8 * n * self.limbs)[:] = out.reshape(-1).view(np.uint8)

    def span_bounds(self, total, locs, ks, keep=None):
        self.log.append("span_bounds")
        return _Bounds(self.log)

    def sparse_aggregate_dev(self, total, locs, ks, vals, zeros, out, sorted_lists=False, bounds=None):
        self.log.append("sparse_aggregate_dev" + ("(bounds)" if bounds is not None else ""))
        L, dense = self.limbs, []
        for loc, k, v, z in zip(locs, ks, vals, zeros):
            dense.append(orc.expand_to_dense(total, self._at(loc, 4 * k).view(np.uint32), np.ascontiguousarray(self._at(v, 8 * k * L).view(np.uint64).reshape(k, L)),
                                             np.array(list(z)[:L], dtype=np.uint64), self.int_bits))
        self._at(out, 8 * total * L)[:] = orc.aggregate_elem(dense, self.int_bits).reshape(-1).view(np.uint8)

    def sparse_encrypt_aggregate_dev(self, it, idx, locs, ks, pts, pt_limbs, zeros, total, n_jobs, cts, agg, bounds=None, position_range=None):
        self.log.append("sparse_encrypt_aggregate_dev")
        for i, k, pt, ct in zip(idx, ks, pts, cts):
            src = self._at(pt, 8 * k * pt_limbs).view(np.uint64).reshape(k, pt_limbs)
            self._at(ct, 8 * k * self.limbs)[:] = orc.encrypt(self.key, it, i, "single", n_jobs, self.int_bits, np.ascontiguousarray(src)).reshape(-1).view(np.uint8)
        log = self.log
        self.log = []
        self.sparse_aggregate_dev(total, locs, ks, cts, zeros, agg)
        self.log = log


class DecliningEngine(SparseEngine):
    """The library declines every shape (FLASHE_ENOTSUP -> False), nothing is written."""

    def quantize_encrypt_sparse_cohort_dev(self, *a, **k):
        self.log.append("quantize_encrypt_sparse_cohort_dev -> False")
        return False


class ChainedEngine(SparseEngine):
    """The chained launch as its contract states it: the staged form's uploads and zeros, no plaintext buffer."""

    def quantize_encrypt_sparse_cohort_dev(self, it, idx, n, n_jobs, layers, srcs, dtypes, element_bits, u, u_stride, zzz, zzz_is_f64, cts, zeros):
        self.log.append("quantize_encrypt_sparse_cohort_dev")
        p, z = self._quantize(n, layers, srcs, dtypes, element_bits, u, u_stride, zzz, zzz_is_f64)
        for c, ct in enumerate(cts):
            out = orc.encrypt(self.key, it, idx[c], "single", n_jobs, self.int_bits, np.ascontiguousarray(p[c].reshape(n, 1)))
            self._at(ct, 8 * (n + 1))[:] = np.concatenate([out.reshape(-1), z[c:c + 1]]).view(np.uint8)
        self._at(zeros, 8 * len(cts))[:] = z.view(np.uint8)
        return True


def _args(b):
    return {"quantize": {"int_bits": b, "batch": False, "element_bits": 16, "padding": True, "secure": True},
            "precompute": {"enable": False, "num_params": 11}, "mask": "dynamic"}


def _round(monkeypatch, engine_cls, b=20, prefer=None, sorted_lists=True, C=3):
    """One round of compact layers given directly -> (front_end, uploads, aggregate, alpha_list, shape_dict, generator state, engine log)."""
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheSparseCohort
    monkeypatch.setattr(cm.FlasheCipher, "_engine_cls", engine_cls)
    monkeypatch.setattr(cm, "N_JOBS", 4)
    ks, total = (4, 1, 30), 400
    g = np.random.Generator(np.random.PCG64(11))
    co = FlasheSparseCohort(_args(b), first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, sparsity=0.1)
    co.prefer_front_end = prefer
    co.set_iter_index(2)
    masks = [np.sort(g.choice(total, sum(ks), replace=False)) for _ in range(C)]
    if not sorted_lists:
        masks[1] = masks[1][::-1].copy()
    assert co.dynamic_masking("single", [m.tolist() for m in masks], total) == "single"
    compact = [{f"l{i}": (g.standard_normal(k) * 0.05).astype(np.float64 if i == 1 else np.float32) for i, k in enumerate(ks)} for _ in range(C)]
    np.random.seed(77)
    up = co.quantize_encrypt(compact=compact, normalize=True)
    assert up.path == "sparse-cohort"
    st = np.random.get_state()
    return (up.front_end, [u.to_host().tobytes() for u in up.uploads], up.aggregate.to_host().tobytes(), [float(a).hex() for a in co.alpha_list],
            dict(co.shape_dict), (st[1].tobytes(), st[2]), list(co.engine.log))


@pytest.mark.parametrize("sorted_lists", [True, False])
def test_a_missing_or_declining_entry_point_runs_the_staged_form(monkeypatch, sorted_lists):
    missing = _round(monkeypatch, SparseEngine, sorted_lists=sorted_lists)
    declined = _round(monkeypatch, DecliningEngine, sorted_lists=sorted_lists)
    chained = _round(monkeypatch, ChainedEngine, sorted_lists=sorted_lists)
    forced = _round(monkeypatch, ChainedEngine, prefer="staged", sorted_lists=sorted_lists)
    assert [r[0] for r in (missing, declined, chained, forced)] == ["staged", "staged", "fused", "staged"]
    for other in (declined, chained, forced):
        assert other[1:6] == missing[1:6]
    # the staged form: one quantise launch into plaintexts, then the encrypts; the fused one: no plaintexts, then the branch's aggregate
    staged_calls = ["quantize_cohort_dev", "span_bounds", "sparse_encrypt_aggregate_dev"] if sorted_lists else \
                   ["quantize_cohort_dev"] + ["encrypt_dev"] * 3 + ["sparse_aggregate_dev"]
    assert missing[6] == staged_calls and forced[6] == staged_calls
    assert declined[6] == ["quantize_encrypt_sparse_cohort_dev -> False"] + staged_calls
    assert chained[6] == ["quantize_encrypt_sparse_cohort_dev"] + (["span_bounds", "sparse_aggregate_dev(bounds)"] if sorted_lists else ["sparse_aggregate_dev"])


@pytest.mark.parametrize("b", [40, 128])
def test_other_widths_never_ask_for_the_chained_launch(monkeypatch, b):
    r = _round(monkeypatch, ChainedEngine, b=b)
    assert r[0] == "staged" and "quantize_encrypt_sparse_cohort_dev" not in r[6]
