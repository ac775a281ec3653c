"""CPU test: plan_cohort's answers for a precompute job's cohort.  Without the cohort's own mask cache the answer stays "per-client" (the
masks are held per client); with it (cohort_masks=True: FlasheCohort.prepare_encrypt ran) the online step is ONE launch from the floats and
the masks at every int_bits, length and cohort size ("prepared-cohort"), or the staged form with a reason that names the cause
("prepared-staged").  On an engine double that records calls: FlasheCohort's mask chain, its one online launch, the fallback when the
library declines and the cache's life.  The new entry points are declared, exported and indexed.  Touches no device."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from flashe_amd.block import plan_cohort

KEY = bytes(range(32))
LIB = os.path.join(ROOT, "flashe_amd", "libflashe_hip.so")
ENTRY_POINTS = ["flashe_cohort_masks_u32_dev", "flashe_quantize_combine_cohort_dev", "flashe_quantize_combine_cohort_u32_dev",
                "flashe_quantize_batch_combine_cohort_dev"]


class _W:
    def __init__(self, layers):
        self.walking_order = sorted(layers)
        self._weights = dict(layers)


def _layer(n, dtype=np.float32):
    return np.broadcast_to(np.zeros((), dtype), (n,))          # (a shape and a dtype: the planner reads nothing else)


def _cohort(sizes, C=10, dtype=np.float32):
    return [_W({f"l{i}": _layer(s, dtype) for i, s in enumerate(sizes)}) for _ in range(C)]


SETTINGS = [dict(int_bits=128, batch=False), dict(int_bits=120, batch=True), dict(int_bits=20, batch=False),
            dict(int_bits=20, batch=False, compact=True, n_jobs=16), dict(int_bits=27, batch=False, compact=True, n_jobs=16),
            dict(int_bits=64, batch=True, element_bits=8)]


@pytest.mark.parametrize("kw", SETTINGS)
@pytest.mark.parametrize("sizes", [[1], [7, 0, 30_000], [3_000_000]])
@pytest.mark.parametrize("C", [1, 10, 129])
def test_precompute_alone_stays_per_client_and_the_cohort_cache_plans_one_launch(kw, sizes, C):
    kw = dict(kw)
    int_bits = kw.pop("int_bits")
    ws = _cohort(sizes, C=C)
    p = plan_cohort(ws, int_bits, 256, num_clients=C, precompute=True, **kw)
    assert p.path == "per-client" and "precomputed masks are held per client" == p.reason
    q = plan_cohort(ws, int_bits, 256, num_clients=C, precompute=True, cohort_masks=True, **kw)
    assert q.path == "prepared-cohort" and "precomputed masks" in q.reason
    assert (q.n, q.n_elems, q.draw_offsets, q.sizes, q.starts) == (p.n, p.n_elems, p.draw_offsets, p.sizes, p.starts)
    assert q.n == sum(sizes) and q.draw_offsets == [c * q.n for c in range(C)]
    if kw.get("batch"):
        bs = int_bits // (kw.get("element_bits", 16) + int(np.ceil(np.log2(C))))
        assert q.n_elems == sum((s + bs - 1) // bs for s in sizes)
    else:
        assert q.n_elems == q.n


def test_the_staged_answers_name_their_cause():
    ws = _cohort([7, 0, 3000], C=3)
    ws[1]._weights["l2"] = _layer(3000, np.float64)
    p = plan_cohort(ws, 128, 256, precompute=True, cohort_masks=True)
    assert p.path == "prepared-staged" and "float64 for some clients only" in p.reason and "compute class" in p.reason
    assert plan_cohort(ws, 128, 256, precompute=True).path == "per-client"
    p = plan_cohort(_cohort([50], C=3), 32, 256, element_bits=12, batch=True, compact=True, n_jobs=16, precompute=True, cohort_masks=True)
    assert p.path == "prepared-staged" and "batched job" in p.reason
    # every layer float64 for all clients shares its rows
    assert plan_cohort(_cohort([7, 3000], C=3, dtype=np.float64), 128, 256, precompute=True, cohort_masks=True).path == "prepared-cohort"
    # the cache exists under the double mask only: the other masks keep their answers
    assert plan_cohort(_cohort([3000], C=3), 128, 256, precompute=True, cohort_masks=True, mask="single").path == "per-client"
    assert plan_cohort(_cohort([3000], C=3), 128, 256, precompute=True, cohort_masks=True, mask="dynamic").path == "per-client"
    # cohort_masks=False changes no answer of the planner
    assert plan_cohort(_cohort([3000], C=3), 128, 256).path == "staged-chain"


def test_refusals_are_unchanged():
    ws = _cohort([7, 300], C=3)
    for kw in (dict(precompute=True), dict(precompute=True, cohort_masks=True)):
        sparse = _cohort([7, 300], C=3)
        sparse[2]._weights["zzz"] = _layer(1)
        sparse[2].walking_order = sorted(sparse[2]._weights)
        with pytest.raises(TypeError, match="client 2: sparse uploads"):
            plan_cohort(sparse, 128, 256, **kw)
        with pytest.raises(TypeError, match="client 0: sparse uploads"):
            plan_cohort(ws, 128, 256, location_masks=True, **kw)
        other = _cohort([7, 300], C=3)
        other[1]._weights["l1"] = _layer(301)
        with pytest.raises(ValueError, match=r"client 1: layer 'l1' has shape \(301,\), client 0's has \(300,\)"):
            plan_cohort(other, 128, 256, **kw)
        missing = _cohort([7, 300], C=3)
        del missing[2]._weights["l0"]
        missing[2].walking_order = ["l1"]
        with pytest.raises(ValueError, match="client 2: layer 'l0' is not a layer of every client"):
            plan_cohort(missing, 128, 256, **kw)
        with pytest.raises(ValueError, match="at least one client"):
            plan_cohort([], 128, 256, **kw)


def test_entry_points_are_declared_exported_and_indexed():
    from flashe_amd import _lib
    header = open(os.path.join(ROOT, "include", "flashe.h")).read()
    index = open(os.path.join(ROOT, "include", "ENTRY_POINTS.md")).read()
    nm = shutil.which("nm")
    exported = subprocess.run([nm, "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout.split() if nm else None
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header, name
        assert f"| `{name}` |" in index, name
        assert name in _lib.EXPORTED_SYMBOLS, name
        if exported is not None:
            assert name in exported, name
    if exported is None:
        import ctypes
        lib = ctypes.CDLL(LIB)
        assert all(hasattr(lib, name) for name in ENTRY_POINTS)


# ------------------------------------------------------------------------------------------------ the cohort on an engine double
class _Buf:
    def __init__(self, engine, nbytes):
        self.engine, self.nbytes, self.ptr = engine, int(nbytes), engine._next
        engine._next += (self.nbytes + 255) & ~255

    def upload_at(self, off, arr):
        assert off + np.asarray(arr).nbytes <= self.nbytes
        return self

    def free(self):
        pass


class RecordingEngine:
    """What a precompute FlasheCohort calls, recorded by name; nothing is computed."""
    answer = True            # what quantize_combine_cohort_dev returns
    limbs, cu_count, device = 2, 2, 0
    PREPARED_ENCRYPT, PREPARED_DECRYPT = 1, 2

    def __init__(self, key, int_bits, device=0, stream=None):
        self.int_bits, self._next, self.log, self.args = int_bits, 1 << 20, [], {}
        self.limbs = 2 if int_bits > 64 else 1

    def _rec(self, name, *a, **kw):
        self.log.append(name)
        self.args[name] = (a, kw)

    def set_key(self, key):
        pass

    def sync(self):
        pass

    def alloc(self, nbytes):
        return _Buf(self, nbytes)

    def alloc_vec(self, n, limbs=None):
        return _Buf(self, max(8 * n * (limbs or self.limbs), 16))

    def hold(self, keep):
        pass

    def compact_supported(self):
        return True

    def prepare_encrypt(self, *a):
        self._rec("prepare_encrypt", *a)

    def prepare_decrypt(self, *a):
        self._rec("prepare_decrypt", *a)

    def prepared_discard(self, which):
        self._rec("prepared_discard", which)

    def cohort_masks_dev(self, *a, **kw):
        self._rec("cohort_masks_dev", *a, **kw)

    def quantize_combine_cohort_dev(self, *a, **kw):
        self._rec("quantize_combine_cohort_dev", *a, **kw)
        return type(self).answer

    def quantize_batch_tensors_dev(self, *a):
        self._rec("quantize_batch_tensors_dev", *a)

    def combine_batch_sum_dev(self, *a):
        self._rec("combine_batch_sum_dev", *a)

    def widen_u32_dev(self, *a):
        self._rec("widen_u32_dev", *a)

    def narrow_u32_dev(self, *a):
        self._rec("narrow_u32_dev", *a)

    def quantize_encrypt_model_dev(self, *a):
        raise AssertionError("no AES in the prepared cohort step")

    quantize_encrypt_cohort_dev = quantize_encrypt_cohort_u32_dev = quantize_batch_encrypt_cohort_dev = encrypt_batch_sum_dev = quantize_encrypt_model_dev
    quantize_encrypt_prepared_model_dev = quantize_encrypt_model_dev      # (the per-client prepared step must not run either)


class DecliningEngine(RecordingEngine):
    answer = False


SIZES = [7, 0, 301]


def _make(monkeypatch, engine_cls, b=128, batch=False, compact=False, C=3, num_params=None):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheCohort
    monkeypatch.setattr(cm.FlasheCipher, "_engine_cls", engine_cls)
    monkeypatch.setattr(cm, "N_JOBS", 16)
    monkeypatch.setenv("FLASHE_DEVICE_RNG", "0")
    bs = b // (16 + int(np.ceil(np.log2(C)))) if batch else 1
    n_ct = sum((s + bs - 1) // bs for s in SIZES)
    args = {"quantize": {"int_bits": b, "batch": batch, "element_bits": 16, "padding": True, "secure": True},
            "precompute": {"enable": True, "num_params": n_ct if num_params is None else num_params}}
    co = FlasheCohort(args, first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, compact=compact)
    co.set_iter_index(4)
    ws = [_W({f"l{i}": np.zeros(s, np.float32) for i, s in enumerate(SIZES)}) for _ in range(C)]
    return co, ws, n_ct


@pytest.mark.parametrize("b, batch, compact", [(128, False, False), (120, True, False), (20, False, False), (20, False, True)])
def test_the_cohort_prepares_one_chain_and_runs_one_online_launch(monkeypatch, b, batch, compact):
    co, ws, n_ct = _make(monkeypatch, RecordingEngine, b=b, batch=batch, compact=compact)
    eng = co.cipher.engine
    assert co.plan(ws).path == "per-client"
    eng.log.clear()
    co.prepare_encrypt()
    assert eng.log[0] == "cohort_masks_dev" and "prepare_encrypt" not in eng.log
    a, kw = eng.args["cohort_masks_dev"]
    assert a[:5] == (5, 0, 3, n_ct, 16) and len(a[5]) == 3 and kw == {"compact": compact}          # iter + 1, first_idx, C, num_params, n_jobs
    assert all(cl.cipher.next_iter_encrypt_prepared == {} for cl in co._clients)
    assert co.plan(ws).path == "prepared-cohort"
    co.set_iter_index(5)
    eng.log.clear()
    np.random.seed(3)
    up = co.quantize_encrypt(ws)
    assert up.path == "prepared-cohort" and eng.log == ["quantize_combine_cohort_dev"]
    a, kw = eng.args["quantize_combine_cohort_dev"]
    assert a[0] == sum(SIZES) and [r[0] for r in a[1]] == [0, 7, 7] and len(a[2]) == 3 and a[4] == 16 and len(a[6]) == 3 and len(a[7]) == 3
    assert kw == {"compact": compact, "batch": (n_ct, 18) if batch else None}
    assert all(len(v) == n_ct for v in up.ciphertexts) and len(up.partial_sum) == n_ct
    assert all(v.elem_bytes == (4 if compact else 8) for v in up.ciphertexts + [up.partial_sum])
    got = np.random.get_state()                                # client-major draws: one stretch of C n values of the stream
    np.random.seed(3)
    np.random.random(3 * sum(SIZES))
    assert np.array_equal(got[1], np.random.get_state()[1]) and got[2] == np.random.get_state()[2]
    # consumed once: the next plan is the clients' own again
    assert co._masks is None and co.plan(ws).path == "per-client"


def test_a_declined_launch_and_the_ab_switch_take_the_staged_form(monkeypatch):
    staged = ["quantize_batch_tensors_dev"] * 3 + ["combine_batch_sum_dev"]
    co, ws, n_ct = _make(monkeypatch, DecliningEngine)
    co.prepare_encrypt()
    eng = co.cipher.engine
    eng.log.clear()
    up = co.quantize_encrypt(ws)
    assert up.path == "prepared-staged" and eng.log == ["quantize_combine_cohort_dev"] + staged and co._masks is None
    a, _kw = eng.args["combine_batch_sum_dev"]
    assert a[0] == n_ct and a[2] == 2 and len(a[3]) == 3 and a[4] is None                    # add = the masks, minus = NULL
    co, ws, n_ct = _make(monkeypatch, RecordingEngine)
    co.prepare_encrypt()
    co.prefer = "staged-chain"
    co.cipher.engine.log.clear()
    assert co.quantize_encrypt(ws).path == "prepared-staged" and co.cipher.engine.log == staged
    # compact: the masks are widened before and the results narrowed after
    co, ws, n_ct = _make(monkeypatch, DecliningEngine, b=20, compact=True)
    co.prepare_encrypt()
    co.cipher.engine.log.clear()
    up = co.quantize_encrypt(ws)
    assert up.path == "prepared-staged"
    assert co.cipher.engine.log == ["quantize_combine_cohort_dev"] + ["quantize_batch_tensors_dev"] * 3 + ["widen_u32_dev"] * 3 + ["combine_batch_sum_dev"] + ["narrow_u32_dev"] * 4
    assert all(v.elem_bytes == 4 for v in up.ciphertexts + [up.partial_sum])


def test_a_cache_of_another_length_raises_where_the_first_client_does_and_stays(monkeypatch):
    co, ws, n_ct = _make(monkeypatch, RecordingEngine, num_params=sum(SIZES) + 1)
    co.prepare_encrypt()
    eng = co.cipher.engine
    eng.log.clear()
    np.random.seed(11)
    with pytest.raises(ValueError, match="could not be broadcast"):
        co.quantize_encrypt(ws)
    got = np.random.get_state()
    np.random.seed(11)
    np.random.random(sum(SIZES))
    assert np.array_equal(got[1], np.random.get_state()[1]) and got[2] == np.random.get_state()[2]
    assert eng.log == [] and co._masks is not None and co.plan(ws).path == "prepared-cohort"
    with pytest.raises(ValueError, match="could not be broadcast"):
        co.quantize_encrypt(ws, seeds=[5, 6, 7])
    got = np.random.get_state()
    np.random.seed(5)
    np.random.random(sum(SIZES))
    assert np.array_equal(got[1], np.random.get_state()[1]) and got[2] == np.random.get_state()[2]


def test_single_mask_and_prepare_decrypt_go_to_the_clients(monkeypatch):
    co, ws, n_ct = _make(monkeypatch, RecordingEngine)
    eng = co.cipher.engine
    eng.log.clear()
    co.prepare_decrypt()
    assert eng.log == ["prepare_decrypt"] and set(co.cipher.next_iter_decrypt_prepared) == {"add", "minus"}
    for cl in co._clients:
        cl.cipher.masking_scheme = "single"
    for cl in co._clients:
        cl.cipher.engine.log.clear()
    co.prepare_encrypt()
    assert co._masks is None and all(cl.cipher.engine.log == ["prepare_encrypt"] for cl in co._clients)
    with pytest.raises(OverflowError):
        co2, _ws, _n = _make(monkeypatch, RecordingEngine)
        co2.lead.cipher.iter_index = 2 ** 32 - 1
        co2.prepare_encrypt()
