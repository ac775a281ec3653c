"""CPU test: plan_cohort(present=...) -- a round in which clients dropped out.  A gapped wide cohort keeps "cohort-chain" while the launch
admits it (present + runs PRF streams, at most 144), every other rule stays, a gapped compact cohort is staged with a reason that names
the cause, present=None and present=everyone give equal plans, and bad lists are refused.  On an engine double that records calls:
FlasheCohort hands the runs entry points the present clients' cipher indices, keeps the add / minus LISTS with the mask, refuses a bad
`present` before any state is touched, and _CohortLead takes the combine pass only for exactly those lists.  Touches no device."""
import numpy as np
import pytest

from flashe_amd.block import cohort_admission_length, compact_cohort_admission_length, plan_cohort
from test_cohort_batch_planner import KEY, RecordingEngine, _W, _layer

CU = 256


def _ws(n, C, dtype=np.float32):
    return [_W({"w": _layer(n, dtype)}) for _ in range(C)]


def _plan(ws, present, int_bits=128, **kw):
    args = dict(element_bits=16, batch=False, mask="double", num_clients=10)
    args.update(kw)
    return plan_cohort(ws, int_bits, CU, present=present, **args)


# ------------------------------------------------------------------------------------------------ plan_cohort
@pytest.mark.parametrize("present,runs", [([0, 1, 3, 4], 2), ([1, 2], 1), ([0, 4], 2), ([0, 2, 4], 3), ([0, 1, 2, 3, 4], 1), ([7], 1)])
def test_a_gapped_wide_cohort_chains(present, runs):
    adm = cohort_admission_length(CU)
    p = _plan(_ws(adm, len(present)), present)
    assert (p.path, p.reason, p.present, p.runs) == ("cohort-chain", "", present, runs)
    assert p.draw_offsets == [c * adm for c in range(len(present))]              # the p-th PRESENT client's draws: absent clients draw nothing
    short = _plan(_ws(adm - 1, len(present)), present)
    assert short.path == "staged-chain" and "fill the chip" in short.reason
    # batched, bs 6 at 120 bits and ten clients: the length rule counts elements
    p = _plan(_ws(6 * adm, len(present)), present, int_bits=120, batch=True)
    assert (p.path, p.n_elems, p.runs) == ("cohort-chain", adm, runs)
    p = _plan(_ws(6 * adm - 6, len(present)), present, int_bits=120, batch=True)
    assert p.path == "staged-chain" and "fill the chip" in p.reason


def test_a_gapped_compact_cohort_is_staged_and_names_the_reason():
    n = compact_cohort_admission_length(CU, 20, 16)
    ws = _ws(n, 4)
    p = _plan(ws, [0, 1, 3, 4], int_bits=20, compact=True, n_jobs=16)
    assert p.path == "staged-chain" and "dropped out" in p.reason and "compact" in p.reason and "2 runs" in p.reason
    assert _plan(ws, [1, 2, 3, 4], int_bits=20, compact=True, n_jobs=16).path == "cohort-chain"          # one run: the compact chain as ever
    assert _plan(ws, None, int_bits=20, compact=True, n_jobs=16).path == "cohort-chain"
    p = _plan(_ws(n - 1, 4), [0, 1, 3, 4], int_bits=20, compact=True, n_jobs=16)                          # the length rule speaks first
    assert p.path == "staged-chain" and "fill the chip" in p.reason


def test_every_other_rule_stays():
    adm = cohort_admission_length(CU)
    ws, present = _ws(adm, 4), [0, 1, 3, 4]
    p = _plan(ws, present, mask="single")
    assert p.path == "staged-chain" and "single mask" in p.reason
    assert _plan(ws, present, chain=False).reason == "FLASHE_CHAIN=0"
    p = _plan(ws, present, precompute=True)
    assert p.path == "per-client" and "precomputed" in p.reason
    assert _plan(ws, present, mask="dynamic").path == "per-client"
    assert _plan(ws, present, int_bits=64).reason == "int_bits <= 64"
    p = _plan(ws, present, int_bits=120, batch=True, element_bits=8)
    assert p.path == "staged-chain" and "bs 10" in p.reason
    mixed = _ws(adm, 4)
    mixed[2]._weights["w"] = _layer(adm, np.float64)
    p = _plan(mixed, present)
    assert p.path == "staged-chain" and "float64 for some clients only" in p.reason
    # a precompute job whose cohort holds the masks: the online launch, given the present clients' masks
    p = _plan(ws, present, precompute=True, cohort_masks=True)
    assert (p.path, p.present, p.runs) == ("prepared-cohort", present, 2)
    p = _plan(ws, present, precompute=True, cohort_masks=True, int_bits=20, compact=True, n_jobs=16)
    assert p.path == "prepared-cohort"
    assert _plan(mixed, present, precompute=True, cohort_masks=True).path == "prepared-staged"


def test_the_stream_limit():
    """present + runs <= 144: 72 singletons fit, 73 do not; 128 clients fit in 16 runs and not in 17."""
    adm = cohort_admission_length(CU)
    one = _ws(adm, 1)
    for C, ok in ((72, True), (73, False)):
        p = _plan(one * C, list(range(0, 2 * C, 2)), num_clients=256)
        assert p.runs == C and (p.path == "cohort-chain") == ok, (C, p.path, p.reason)
    assert "144" in p.reason and "73 runs" in p.reason
    for runs, ok in ((16, True), (17, False)):
        present, at = [], 0
        for c in range(128):
            present.append(at)
            at += 2 if c % 7 == 6 and c // 7 + 1 < runs else 1          # a gap behind every seventh client, runs - 1 of them
        p = _plan(one * 128, present, num_clients=256)
        assert p.runs == runs and (p.path == "cohort-chain") == ok, (runs, p.path, p.reason)


def test_present_none_and_everyone_give_equal_plans():
    adm = cohort_admission_length(CU)
    for kw in ({}, {"int_bits": 120, "batch": True}, {"int_bits": 20, "compact": True, "n_jobs": 16}, {"mask": "single"},
               {"precompute": True, "cohort_masks": True}):
        a, b = _plan(_ws(adm + 3, 5), None, **kw), _plan(_ws(adm + 3, 5), [0, 1, 2, 3, 4], **kw)
        assert vars(a) == vars(b), kw
        assert a.present == [0, 1, 2, 3, 4] and a.runs == 1


@pytest.mark.parametrize("present", [[1, 0, 2], [0, 0, 1], [0, 1], [0, 1, 2, 3], [-1, 0, 1], [0, 1.5, 2], ["a", "b", "c"], 5])
def test_bad_present_lists_are_refused(present):
    with pytest.raises(ValueError, match="present"):
        _plan(_ws(1000, 3), present)


# ------------------------------------------------------------------------------------------------ the cohort on an engine double
class RunsEngine(RecordingEngine):
    def quantize_encrypt_cohort_runs_dev(self, *a):
        self._rec("quantize_encrypt_cohort_runs_dev", *a)
        return type(self).answer

    def quantize_batch_encrypt_cohort_runs_dev(self, *a):
        self._rec("quantize_batch_encrypt_cohort_runs_dev", *a)
        return type(self).answer

    def quantize_encrypt_cohort_dev(self, *a):
        self._rec("quantize_encrypt_cohort_dev", *a)
        return type(self).answer

    def quantize_batch_tensors_dev(self, *a):
        self._rec("quantize_batch_tensors_dev", *a)

    def combine_unquantize_model_dev(self, *a):
        self._rec("combine_unquantize_model_dev", *a)

    def decrypt_unquantize_model_dev(self, *a):
        self._rec("decrypt_unquantize_model_dev", *a)


class DecliningRunsEngine(RunsEngine):
    answer = False


def _args(b, batch):
    return {"quantize": {"int_bits": b, "batch": batch, "element_bits": 16, "padding": True, "secure": True}, "precompute": {"enable": False}}


def _cohort(monkeypatch, engine_cls, b=128, batch=False, first_idx=0, n_local=5, num_clients=5):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheCohort
    monkeypatch.setattr(cm.FlasheCipher, "_engine_cls", engine_cls)
    monkeypatch.setattr(cm, "N_JOBS", 16)
    monkeypatch.setenv("FLASHE_DEVICE_RNG", "0")
    co = FlasheCohort(_args(b, batch), first_idx=first_idx, n_local=n_local, num_clients=num_clients, prp_seed=KEY)
    co.set_iter_index(4)
    return co


def _models(n_values, C):
    return [_W({"a": np.zeros(7, np.float32), "b": np.zeros(n_values - 7, np.float32)}) for _ in range(C)]


@pytest.mark.parametrize("batch", [False, True])
def test_the_cohort_hands_the_launch_the_present_indices_and_keeps_the_lists(monkeypatch, batch):
    adm = cohort_admission_length(RunsEngine.cu_count)
    b, name = (120, "quantize_batch_encrypt_cohort_runs_dev") if batch else (128, "quantize_encrypt_cohort_runs_dev")
    n = 7 + 6 * adm if batch else adm + 8                       # (batched: 2 + adm elements at bs 6)
    co = _cohort(monkeypatch, RunsEngine, b, batch)
    np.random.seed(3)
    up = co.quantize_encrypt(_models(n, 4), present=[0, 1, 3, 4])
    eng = co.cipher.engine
    assert up.path == "cohort-chain" and eng.log == [name] and up.present == [0, 1, 3, 4] and len(up.ciphertexts) == 4
    a = eng.args[name]
    assert a[:2] == (4, [0, 1, 3, 4]) and len(a[5 if batch else 4]) == 2 and len(a[6 if batch else 5]) == 4          # iter, idx, shared rows, source rows
    assert a[-1] is not None                                   # the whole federation: a decrypt mask
    m = co.lead._cohort_mask
    assert m[2:] == (4, [2, 5], [0, 3]) and len(m[1]) == len(up.partial_sum)
    # another federation offset, every stream a run boundary
    co = _cohort(monkeypatch, RunsEngine, b, batch, first_idx=10, n_local=5, num_clients=20)
    up = co.quantize_encrypt(_models(n, 3), present=[0, 2, 4])
    assert co.cipher.engine.args[name][1] == [10, 12, 14] and up.present == [10, 12, 14]
    assert co.cipher.engine.args[name][-1] is None and co.lead._cohort_mask is None           # clients outside the cohort: no mask
    # present=None is the call it always was
    co = _cohort(monkeypatch, RunsEngine, b, batch)
    up = co.quantize_encrypt(_models(n, 5))
    old = "quantize_batch_encrypt_cohort_dev" if batch else "quantize_encrypt_cohort_dev"
    assert co.cipher.engine.log == [old] and co.cipher.engine.args[old][1] == 0 and up.present == [0, 1, 2, 3, 4]
    assert co.lead._cohort_mask[3:] == ([5], [0])


def test_the_library_declining_runs_the_staged_form_with_the_gapped_indices(monkeypatch):
    adm = cohort_admission_length(RunsEngine.cu_count)
    co = _cohort(monkeypatch, DecliningRunsEngine)
    np.random.seed(3)
    up = co.quantize_encrypt(_models(adm + 8, 4), present=[0, 1, 3, 4])
    eng = co.cipher.engine
    assert up.path == "staged-chain" and eng.log == ["quantize_encrypt_cohort_runs_dev"] + ["quantize_batch_tensors_dev"] * 4 + ["encrypt_batch_sum_dev"]
    assert eng.args["encrypt_batch_sum_dev"][1] == [0, 1, 3, 4] and co.lead._cohort_mask is None and up.present == [0, 1, 3, 4]
    # a tiny model never asks
    co = _cohort(monkeypatch, RunsEngine)
    up = co.quantize_encrypt(_models(100, 4), present=[0, 1, 3, 4])
    assert up.path == "staged-chain" and co.cipher.engine.log == ["quantize_batch_tensors_dev"] * 4 + ["encrypt_batch_sum_dev"]


@pytest.mark.parametrize("present,n_w", [([1, 0], 2), ([0, 0], 2), ([0, 5], 2), ([0, 1], 3), ([-1, 0], 2), ([], 0)])
def test_a_bad_present_is_refused_before_any_state_is_touched(monkeypatch, present, n_w):
    co = _cohort(monkeypatch, RunsEngine)
    co._last, co.lead._cohort_mask = "last", "mask"
    q = co.quantizer
    before = (q.alpha_list, q.r_max_list, co.shape_dict)
    np.random.seed(11)
    state = np.random.get_state()
    with pytest.raises(ValueError):
        co.quantize_encrypt(_models(100, n_w), present=present)
    with pytest.raises(ValueError, match="seeds"):
        co.quantize_encrypt(_models(100, 2), present=[0, 3], seeds=[1, 2, 3])
    after = np.random.get_state()
    assert after[0] == state[0] and after[2] == state[2] and np.array_equal(after[1], state[1])
    assert co.cipher.engine.log == [] and (co._last, co.lead._cohort_mask) == ("last", "mask")
    assert (q.alpha_list, q.r_max_list, co.shape_dict) == before


def test_the_lead_takes_the_combine_pass_only_for_exactly_the_kept_lists(monkeypatch):
    adm = cohort_admission_length(RunsEngine.cu_count)
    co = _cohort(monkeypatch, RunsEngine)
    np.random.seed(3)
    up = co.quantize_encrypt(_models(adm + 8, 4), present=[0, 1, 3, 4])
    ld, eng, sizes = co.lead, co.cipher.engine, [7, adm + 1]
    ld.quantizer.alpha_list = [0.5, 0.5]

    def run(add, minus):
        eng.log.clear()
        ld._decrypt_floats(up.partial_sum, sizes, None, add, minus)
        return list(eng.log)

    assert run([2, 5], [0, 3]) == ["combine_unquantize_model_dev"]
    a = eng.args["combine_unquantize_model_dev"]
    assert a[1] is up.partial_sum.buf and a[2] is ld._cohort_mask[1].buf and a[3] is None
    launch = ["decrypt_unquantize_model_dev"]
    assert run([5], [0]) == launch                             # everyone: not what this upload's mask stands for
    assert run([2, 5], [0]) == launch
    assert run([5, 2], [0, 3]) == launch
    assert run([2], [0]) == launch
