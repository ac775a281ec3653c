"""CPU test: plan_cohort's cut=True rule (FlasheCohort(cut=True), flashe_quantize_encrypt_cohort_cut_dev and its _u32 form) -- "cut-chain"
exactly where the only obstacle was "the vector does not fill the chip uncut", every other rule and reason as it was, cut=False today's
plans -- and the launches FlasheCohort makes on an engine double defined here: one call of the cut launch in place of C quantise passes
and the summed batch encrypt.  Touches no device and no library."""
import numpy as np
import pytest

from flashe_amd.block import (cohort_admission_length, cohort_cut_items, cohort_cut_parts, compact_cohort_admission_length, plan_cohort)

KEY = bytes(range(32))
CU = 80
WIDTHS = (16, 20, 23, 24, 32)


class _W:
    def __init__(self, layers):
        self.walking_order = sorted(layers)
        self._weights = dict(layers)


def _layer(n, dtype=np.float32):
    return np.broadcast_to(np.zeros((), dtype), (n,))          # (a shape and a dtype: the planner reads nothing else)


def _ws(n, C=5, dtype=np.float32):
    head = min(n, 300)
    return [_W({"a": _layer(head, dtype), "b": _layer(0), "c": _layer(n - head)}) for _ in range(C)]


def _key(p):
    return (p.path, p.reason, p.n, p.n_elems, p.draw_offsets, p.present, p.runs)


# ------------------------------------------------------------------------------------------------ the planner
@pytest.mark.parametrize("C", [1, 3, 17, 128])
@pytest.mark.parametrize("n", [1, 255, 700, 61706])
def test_a_short_wide_cohort_plans_the_cut_chain(C, n):
    for b in (65, 120, 128):
        old = plan_cohort(_ws(n, C), b, CU)
        assert (old.path, old.reason, old.parts) == ("staged-chain", "the vector does not fill the chip uncut", 1)
        p = plan_cohort(_ws(n, C), b, CU, cut=True)
        assert (p.path, p.reason) == ("cut-chain", "")
        assert p.parts == cohort_cut_parts(C, cohort_cut_items(n, b, 16), CU) and 1 <= p.parts <= min(16, C)
        assert _key(p)[2:] == _key(old)[2:]


@pytest.mark.parametrize("b", WIDTHS)
def test_a_short_compact_cohort_plans_the_cut_chain(b):
    adm = compact_cohort_admission_length(CU, b, 16)
    for n in (1, 5, 700, adm - 1):
        old = plan_cohort(_ws(n), b, CU, compact=True, n_jobs=16)
        assert (old.path, old.reason) == ("staged-chain", "the vector does not fill the chip uncut")
        p = plan_cohort(_ws(n), b, CU, compact=True, n_jobs=16, cut=True)
        assert (p.path, p.reason) == ("cut-chain", "") and p.parts == cohort_cut_parts(5, cohort_cut_items(n, b, 16, True), CU)
    # from the admission length on the uncut chain runs, cut or not
    for cut in (False, True):
        assert plan_cohort(_ws(adm), b, CU, compact=True, n_jobs=16, cut=cut).path == "cohort-chain"


def test_the_edges_of_the_length_rule():
    adm = cohort_admission_length(CU)
    below, at = plan_cohort(_ws(adm - 1, 3), 128, CU, cut=True), plan_cohort(_ws(adm, 3), 128, CU, cut=True)
    assert (below.path, below.parts) == ("cut-chain", 1)       # more than half an item per wave: one piece, no combine pass
    assert (at.path, at.reason, at.parts) == ("cohort-chain", "", 1)
    # a vector that is too LONG is no shape of the cut chain either (one counter window)
    assert plan_cohort(_ws(2 ** 32, 2), 20, CU, compact=True, cut=True).path == "staged-chain"
    # an empty model has nothing to launch
    assert plan_cohort(_ws(0, 2), 128, CU, cut=True).path == "staged-chain"
    # config 3's shape on the chip it was measured on: 61,706 values are 484 half tiles, eight pieces of them fill the 4,096 waves once
    p = plan_cohort(_ws(61706, 100), 128, 256, cut=True)
    assert (p.path, p.parts) == ("cut-chain", 8)
    assert plan_cohort(_ws(61706, 128), 128, 256, cut=True).parts == 8 and plan_cohort(_ws(700, 128), 128, 256, cut=True).parts == 16
    assert plan_cohort(_ws(700, 40), 128, 256, cut=True).parts == 10 and plan_cohort(_ws(700, 17), 128, 256, cut=True).parts == 4
    assert [plan_cohort(_ws(700, C), 128, 256, cut=True).parts for C in (1, 2, 3, 7, 8)] == [1, 1, 1, 1, 2]


def test_every_other_reason_still_wins():
    n = 700
    for kw, b, path, reason in (
            ({"mask": "single"}, 128, "staged-chain", "single mask"),
            ({"mask": "other"}, 128, "per-client", "mask 'other'"),
            ({"precompute": True}, 128, "per-client", "precomputed"),
            ({"chain": False}, 128, "staged-chain", "FLASHE_CHAIN=0"),
            ({}, 64, "staged-chain", "int_bits <= 64"),
            ({}, 33, "staged-chain", "int_bits <= 64"),
            ({"compact": True}, 21, "staged-chain", "int_bits 21 is not a width of the compact chain"),
            ({"compact": True, "batch": True, "element_bits": 12}, 32, "staged-chain", "batched job"),
            ({"batch": True, "element_bits": 4}, 128, "staged-chain", "batched job with bs"),
            ({"precompute": True, "cohort_masks": True}, 128, "prepared-cohort", "precomputed masks")):
        old, new = plan_cohort(_ws(n), b, CU, **kw), plan_cohort(_ws(n), b, CU, cut=True, **kw)
        assert (new.path, new.parts) == (path, 1) and reason in new.reason, (kw, new.path, new.reason)
        assert vars(new) == vars(old), kw
    # more than 128 clients
    new = plan_cohort(_ws(n, 129), 128, CU, cut=True)
    assert new.path == "staged-chain" and "128 clients" in new.reason and vars(new) == vars(plan_cohort(_ws(n, 129), 128, CU))
    assert plan_cohort(_ws(n, 128), 128, CU, cut=True).path == "cut-chain"
    # a short BATCHED cohort whose bs the chained launch packs: still the length rule, and the cut chain does not batch
    new = plan_cohort(_ws(n), 128, CU, batch=True, cut=True)
    assert new.path == "staged-chain" and new.reason.startswith("the vector does not fill the chip uncut") and "batched" in new.reason
    # a layer that is float64 for some clients only
    mixed = _ws(n)
    mixed[1]._weights["a"] = _layer(300, np.float64)
    new = plan_cohort(mixed, 128, CU, cut=True)
    assert (new.path, new.reason) == ("staged-chain", "a layer is float64 for some clients only")
    assert plan_cohort(_ws(n, dtype=np.float64), 128, CU, cut=True).path == "cut-chain"       # (float64 for all: a shared row)
    # clients dropped out: several runs
    for kw, b in (({}, 128), ({"compact": True}, 20), ({"compact": True, "compact_runs": True}, 20)):
        new = plan_cohort(_ws(n, 4), b, CU, present=[0, 1, 3, 4], cut=True, **kw)
        assert new.path == "staged-chain" and "2 runs" in new.reason and "one run" in new.reason, kw
        assert plan_cohort(_ws(n, 3), b, CU, present=[1, 2, 3], cut=True, **kw).path == "cut-chain"
        assert vars(plan_cohort(_ws(n, 3), b, CU, present=[0, 1, 2], cut=True, **kw)) == vars(plan_cohort(_ws(n, 3), b, CU, cut=True, **kw))


@pytest.mark.parametrize("b", [16, 20, 64, 65, 128])
def test_cut_false_is_todays_plan_and_long_vectors_do_not_change(b):
    adm = cohort_admission_length(CU)
    for n in (1, 700, adm - 1, adm, compact_cohort_admission_length(CU, 16, 16) + 5):
        for kw in ({}, {"mask": "single"}, {"precompute": True}, {"chain": False}, {"batch": True, "element_bits": 4}, {"compact": b <= 32}):
            a = plan_cohort(_ws(n), b, CU, **kw)
            e = plan_cohort(_ws(n), b, CU, cut=False, **kw)
            assert vars(a) == vars(e) and a.parts == 1 and a.path != "cut-chain"
            c = plan_cohort(_ws(n), b, CU, cut=True, **kw)
            if "fill the chip" not in a.reason:
                assert vars(c) == vars(a), (n, kw)


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


class StagedEngine:
    """What FlasheCohort.quantize_encrypt calls on an engine WITHOUT the cut launch, recorded by name; nothing is computed."""
    limbs, cu_count, device = 2, 2, 0

    def __init__(self, key, int_bits, device=0, stream=None):
        self.int_bits, self._next, self.log, self.args, self.allocs = int_bits, 1 << 20, [], {}, []

    def set_key(self, key):
        pass

    def alloc(self, nbytes):
        self.allocs.append(int(nbytes))
        return _Buf(self, nbytes)

    def alloc_vec(self, n, limbs=None):
        return _Buf(self, max(8 * n * (limbs or self.limbs), 16))

    def hold(self, keep):
        pass

    def _rec(self, name, *a):
        self.log.append(name)
        self.args[name] = a

    def quantize_encrypt_model_dev(self, *a):
        raise AssertionError("not a call of the cohort")

    def quantize_encrypt_cohort_dev(self, *a):
        raise AssertionError("the uncut launch for a short vector")

    def quantize_batch_tensors_dev(self, *a):
        self._rec("quantize_batch_tensors_dev", *a)

    def encrypt_batch_sum_dev(self, *a):
        self._rec("encrypt_batch_sum_dev", *a)

    def combine_unquantize_model_dev(self, *a):
        self._rec("combine_unquantize_model_dev", *a)


class CutEngine(StagedEngine):
    answer, parts = True, 3

    def cohort_cut_parts(self, n_clients, n, n_jobs, compact=False):
        assert not compact
        return type(self).parts

    def quantize_encrypt_cohort_cut_dev(self, *a):
        self._rec("quantize_encrypt_cohort_cut_dev", *a)
        return type(self).answer


class OnePieceEngine(CutEngine):
    parts = 1


class DecliningCutEngine(CutEngine):
    answer = False


class NoShapeEngine(CutEngine):
    parts = 0

    def quantize_encrypt_cohort_cut_dev(self, *a):
        raise AssertionError("the library gave no pieces: nothing to launch")


def _args(b=128):
    return {"quantize": {"int_bits": b, "batch": False, "element_bits": 16, "padding": True, "secure": True}, "precompute": {"enable": False}}


def _cohort(monkeypatch, engine_cls, cut=True, n_local=5, num_clients=5, first_idx=0):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheCohort
    monkeypatch.setattr(cm.FlasheCipher, "_engine_cls", engine_cls)
    monkeypatch.setattr(cm, "N_JOBS", 16)
    monkeypatch.setenv("FLASHE_DEVICE_RNG", "0")
    co = FlasheCohort(_args(), first_idx=first_idx, n_local=n_local, num_clients=num_clients, prp_seed=KEY, cut=cut)
    co.set_iter_index(4)
    return co


def _models(n, C):
    return [_W({"a": np.zeros(7, np.float32), "b": np.zeros(n - 7, np.float32)}) for _ in range(C)]


STAGED_LOG = ["quantize_batch_tensors_dev"] * 5 + ["encrypt_batch_sum_dev"]
N = 700


def test_the_cut_cohort_is_one_call_and_keeps_the_mask(monkeypatch):
    co = _cohort(monkeypatch, CutEngine)
    np.random.seed(3)
    up = co.quantize_encrypt(_models(N, 5))
    eng = co.cipher.engine
    assert up.path == "cut-chain" and eng.log == ["quantize_encrypt_cohort_cut_dev"] and len(up.ciphertexts) == 5
    a = eng.args["quantize_encrypt_cohort_cut_dev"]
    assert a[:4] == (4, 0, N, 16) and len(a[4]) == 2 and len(a[5]) == 5            # iter, first_idx, n, n_jobs, shared rows, source rows
    mask, scratch = a[-2], a[-1]
    assert mask is not None and scratch is not None and scratch.nbytes >= 3 * N * 16 * 2        # three pieces' sums and masks
    m = co.lead._cohort_mask
    assert m[0] == up.partial_sum.ptr and m[2:] == (4, [5], [0]) and len(m[1]) == N
    # the decrypt of the cohort's own sum is the one combine + unquantise pass
    eng.log.clear()
    co.lead.quantizer.alpha_list = [0.5, 0.5]
    co.lead._decrypt_floats(up.partial_sum, [7, N - 7], None, [5], [0])
    assert eng.log == ["combine_unquantize_model_dev"]
    # the scratch is kept for the next round
    before = list(eng.allocs)
    eng.log.clear()
    co.set_iter_index(5)
    assert co.quantize_encrypt(_models(N, 5)).path == "cut-chain" and eng.args["quantize_encrypt_cohort_cut_dev"][-1] is scratch
    assert 3 * N * 16 * 2 not in eng.allocs[len(before):]
    # present = everyone is the same call; a cohort inside a larger federation keeps no mask and needs half the scratch
    co = _cohort(monkeypatch, CutEngine)
    assert co.quantize_encrypt(_models(N, 5), present=[0, 1, 2, 3, 4]).path == "cut-chain" and co.cipher.engine.log == ["quantize_encrypt_cohort_cut_dev"]
    co = _cohort(monkeypatch, CutEngine, n_local=5, num_clients=9, first_idx=3)
    up = co.quantize_encrypt(_models(N, 3), present=[1, 2, 3])
    a = co.cipher.engine.args["quantize_encrypt_cohort_cut_dev"]
    assert up.path == "cut-chain" and a[1] == 4 and a[-2] is None and a[-1].nbytes >= 3 * N * 16 and co.lead._cohort_mask is None
    assert up.present == [4, 5, 6]


def test_one_piece_needs_no_scratch(monkeypatch):
    co = _cohort(monkeypatch, OnePieceEngine)
    up = co.quantize_encrypt(_models(N, 5))
    assert up.path == "cut-chain" and co.cipher.engine.args["quantize_encrypt_cohort_cut_dev"][-1] is None and co._cut_scratch is None


def test_without_the_call_or_without_cut_the_staged_form_runs(monkeypatch):
    for cls, cut in ((StagedEngine, True), (CutEngine, False), (StagedEngine, False)):
        co = _cohort(monkeypatch, cls, cut=cut)
        plan = co.plan(_models(N, 5))
        assert (plan.path, plan.reason, plan.parts) == ("staged-chain", "the vector does not fill the chip uncut", 1)
        up = co.quantize_encrypt(_models(N, 5))
        assert up.path == "staged-chain" and co.cipher.engine.log == STAGED_LOG and co.lead._cohort_mask is None


def test_prefer_staged_never_asks_and_a_declining_library_falls_back(monkeypatch):
    co = _cohort(monkeypatch, CutEngine)
    co.prefer = "staged-chain"
    assert co.plan(_models(N, 5)).path == "cut-chain"
    up = co.quantize_encrypt(_models(N, 5))
    assert up.path == "staged-chain" and co.cipher.engine.log == STAGED_LOG
    co = _cohort(monkeypatch, DecliningCutEngine)
    up = co.quantize_encrypt(_models(N, 5))
    assert up.path == "staged-chain" and co.cipher.engine.log == ["quantize_encrypt_cohort_cut_dev"] + STAGED_LOG and co.lead._cohort_mask is None
    co = _cohort(monkeypatch, NoShapeEngine)
    up = co.quantize_encrypt(_models(N, 5))
    assert up.path == "staged-chain" and co.cipher.engine.log == STAGED_LOG
    # gapped: the staged form with the present clients' indices
    co = _cohort(monkeypatch, CutEngine)
    up = co.quantize_encrypt(_models(N, 4), present=[0, 1, 3, 4])
    assert up.path == "staged-chain" and co.cipher.engine.log == ["quantize_batch_tensors_dev"] * 4 + ["encrypt_batch_sum_dev"]
    assert co.cipher.engine.args["encrypt_batch_sum_dev"][1] == [0, 1, 3, 4]
    # a layer that is float64 for some clients only
    co = _cohort(monkeypatch, CutEngine)
    ws = _models(N, 5)
    ws[2]._weights["a"] = np.zeros(7, np.float64)
    assert co.quantize_encrypt(ws).path == "staged-chain" and "quantize_encrypt_cohort_cut_dev" not in co.cipher.engine.log
