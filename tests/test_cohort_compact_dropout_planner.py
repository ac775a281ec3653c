"""CPU test: plan_cohort(compact_runs=...) -- a COMPACT cohort round in which clients dropped out, on an engine that has the gapped compact
launch (flashe_quantize_encrypt_cohort_runs_u32_dev).  compact_runs=True lets a gapped compact cohort through to the 144-stream rule, every
other rule speaks as before; the default keyword answers what plan_cohort always answered; present=None and present=everyone plan equal
either way.  On an engine double that records calls: FlasheCohort asks compact_runs of the engine, hands the new launch the present clients'
cipher indices and keeps no mask, and an engine double without the method plans and runs as before.  Touches no device."""
import numpy as np
import pytest

from flashe_amd.block import compact_cohort_admission_length, plan_cohort
from test_cohort_batch_planner import KEY, RecordingEngine, _W, _layer

CU = 256
ADM = compact_cohort_admission_length(CU, 20, 16)


def _ws(n, C, dtype=np.float32):
    return [_W({"w": _layer(n, dtype)}) for _ in range(C)]


def _plan(ws, present, int_bits=20, **kw):
    args = dict(element_bits=16, batch=False, mask="double", num_clients=10, compact=True, n_jobs=16)
    args.update(kw)
    return plan_cohort(ws, int_bits, CU, present=present, **args)


# ------------------------------------------------------------------------------------------------ plan_cohort
def test_a_gapped_compact_cohort_chains_on_an_engine_with_the_launch():
    p = _plan(_ws(ADM, 4), [0, 1, 3, 4], compact_runs=True)
    assert (p.path, p.reason, p.present, p.runs) == ("cohort-chain", "", [0, 1, 3, 4], 2)
    assert p.draw_offsets == [c * ADM for c in range(4)]
    short = _plan(_ws(ADM - 1, 4), [0, 1, 3, 4], compact_runs=True)               # one value below the admission length: the length rule speaks
    assert short.path == "staged-chain" and "fill the chip" in short.reason


def test_the_stream_limit_decides_next():
    one = _ws(ADM, 1)
    for C, ok in ((72, True), (73, False)):
        p = _plan(one * C, list(range(0, 2 * C, 2)), num_clients=256, compact_runs=True)
        assert p.runs == C and (p.path == "cohort-chain") == ok, (C, p.path, p.reason)
    assert "144" in p.reason and "73 runs" in p.reason


def test_the_other_rules_stay():
    ws, present = _ws(ADM, 4), [0, 1, 3, 4]
    p = _plan(ws, present, int_bits=21, compact_runs=True)
    assert p.path == "staged-chain" and "not a width of the compact chain" in p.reason and "(16, 20, 23, 24, 32)" in p.reason
    p = _plan(ws, present, batch=True, compact_runs=True)
    assert (p.path, p.reason) == ("staged-chain", "batched job")
    p = _plan(ws, present, mask="single", compact_runs=True)
    assert p.path == "staged-chain" and "single mask" in p.reason
    assert _plan(ws, present, chain=False, compact_runs=True).reason == "FLASHE_CHAIN=0"
    assert _plan(ws, present, precompute=True, compact_runs=True).path == "per-client"
    assert _plan(ws, present, precompute=True, cohort_masks=True, compact_runs=True).path == "prepared-cohort"
    mixed = _ws(ADM, 4)
    mixed[2]._weights["w"] = _layer(ADM, np.float64)
    p = _plan(mixed, present, compact_runs=True)
    assert p.path == "staged-chain" and "float64 for some clients only" in p.reason
    # the wide chain never asked
    wide = dict(int_bits=128, compact=False)
    assert vars(_plan(ws, present, compact_runs=True, **wide)) == vars(_plan(ws, present, **wide))


CASES = [(4, [0, 1, 3, 4], {}), (4, [1, 2, 3, 4], {}), (4, None, {}), (3, [0, 2, 4], {"int_bits": 23}), (4, [0, 1, 3, 4], {"int_bits": 21}),
         (4, [0, 1, 3, 4], {"batch": True}), (4, [0, 1, 3, 4], {"int_bits": 128, "compact": False}), (4, [0, 1, 3, 4], {"mask": "single"})]


@pytest.mark.parametrize("C,present,kw", CASES)
def test_the_default_keyword_answers_as_before(C, present, kw):
    """compact_runs=False is the default, and under it a gapped compact cohort is staged with the reason plan_cohort always gave."""
    for n in (ADM, ADM - 1):
        a, b = _plan(_ws(n, C), present, **kw), _plan(_ws(n, C), present, compact_runs=False, **kw)
        assert vars(a) == vars(b), (n, kw)
    p = _plan(_ws(ADM, 4), [0, 1, 3, 4])
    assert p.path == "staged-chain" and "dropped out" in p.reason and "compact" in p.reason and "2 runs" in p.reason


@pytest.mark.parametrize("compact_runs", [False, True])
def test_present_none_and_everyone_give_equal_plans(compact_runs):
    for kw in ({}, {"int_bits": 23}, {"int_bits": 21}, {"batch": True}, {"int_bits": 128, "compact": False}):
        a = _plan(_ws(ADM + 3, 5), None, compact_runs=compact_runs, **kw)
        b = _plan(_ws(ADM + 3, 5), [0, 1, 2, 3, 4], compact_runs=compact_runs, **kw)
        assert vars(a) == vars(b), kw
        assert a.present == [0, 1, 2, 3, 4] and a.runs == 1
    # one run plans the same with and without the launch
    assert vars(_plan(_ws(ADM, 5), None, compact_runs=True)) == vars(_plan(_ws(ADM, 5), None))


# ------------------------------------------------------------------------------------------------ the cohort on an engine double
class OldCompactEngine(RecordingEngine):
    """An engine from before the gapped compact launch."""

    def compact_supported(self):
        return True

    def quantize_encrypt_cohort_u32_dev(self, *a):
        self._rec("quantize_encrypt_cohort_u32_dev", *a)
        return type(self).answer

    def quantize_batch_tensors_dev(self, *a):
        self._rec("quantize_batch_tensors_dev", *a)

    def narrow_u32_dev(self, *a):
        self._rec("narrow_u32_dev", *a)

    def encrypt_batch_sum_u32_dev(self, *a):
        self._rec("encrypt_batch_sum_u32_dev", *a)

    def decrypt_unquantize_model_dev(self, *a):
        self._rec("decrypt_unquantize_model_dev", *a)


class RunsCompactEngine(OldCompactEngine):
    def quantize_encrypt_cohort_runs_u32_dev(self, *a):
        self._rec("quantize_encrypt_cohort_runs_u32_dev", *a)
        return type(self).answer


def _args(b):
    return {"quantize": {"int_bits": b, "batch": False, "element_bits": 16, "padding": True, "secure": True}, "precompute": {"enable": False}}


def _cohort(monkeypatch, engine_cls, first_idx=0, n_local=5, num_clients=5):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheCohort
    monkeypatch.setattr(cm.FlasheCipher, "_engine_cls", engine_cls)
    monkeypatch.setattr(cm, "N_JOBS", 16)
    monkeypatch.setenv("FLASHE_DEVICE_RNG", "0")
    co = FlasheCohort(_args(20), first_idx=first_idx, n_local=n_local, num_clients=num_clients, prp_seed=KEY, compact=True)
    co.set_iter_index(4)
    return co


def _models(n_values, C):
    return [_W({"a": np.zeros(7, np.float32), "b": np.zeros(n_values - 7, np.float32)}) for _ in range(C)]


def test_the_cohort_asks_the_engine_and_hands_the_launch_the_present_indices(monkeypatch):
    n = compact_cohort_admission_length(RunsCompactEngine.cu_count, 20, 16) + 9
    name = "quantize_encrypt_cohort_runs_u32_dev"
    co = _cohort(monkeypatch, RunsCompactEngine, first_idx=10, n_local=5, num_clients=20)
    ws = _models(n, 4)
    assert co.plan(ws, present=[0, 1, 3, 4]).path == "cohort-chain"
    np.random.seed(3)
    up = co.quantize_encrypt(ws, present=[0, 1, 3, 4])
    eng = co.cipher.engine
    assert up.path == "cohort-chain" and eng.log == [name] and up.present == [10, 11, 13, 14] and len(up.ciphertexts) == 4
    a = eng.args[name]
    assert a[:4] == (4, [10, 11, 13, 14], n, 16) and len(a[4]) == 2 and len(a[5]) == 4           # iter, idx, n, n_jobs, shared rows, source rows
    assert len(a) == 11 and co.lead._cohort_mask is None                                        # no mask at the compact widths
    # the whole federation: still no mask
    co = _cohort(monkeypatch, RunsCompactEngine)
    up = co.quantize_encrypt(_models(n, 3), present=[0, 2, 4])
    assert co.cipher.engine.args[name][1] == [0, 2, 4] and co.lead._cohort_mask is None and up.path == "cohort-chain"
    # present=None is the call it always was
    co = _cohort(monkeypatch, RunsCompactEngine)
    up = co.quantize_encrypt(_models(n, 5))
    assert co.cipher.engine.log == ["quantize_encrypt_cohort_u32_dev"] and co.cipher.engine.args["quantize_encrypt_cohort_u32_dev"][1] == 0
    # prefer = "staged-chain" never asks
    co = _cohort(monkeypatch, RunsCompactEngine)
    co.prefer = "staged-chain"
    up = co.quantize_encrypt(_models(n, 4), present=[0, 1, 3, 4])
    assert up.path == "staged-chain" and name not in co.cipher.engine.log


def test_an_engine_without_the_launch_plans_and_runs_as_before(monkeypatch):
    n = compact_cohort_admission_length(OldCompactEngine.cu_count, 20, 16) + 9
    co = _cohort(monkeypatch, OldCompactEngine)
    ws = _models(n, 4)
    p = co.plan(ws, present=[0, 1, 3, 4])
    assert p.path == "staged-chain" and "compact" in p.reason
    up = co.quantize_encrypt(ws, present=[0, 1, 3, 4])
    assert up.path == "staged-chain" and "quantize_encrypt_cohort_u32_dev" not in co.cipher.engine.log
    # one run given by `present`: the one-run launch with the first index
    co = _cohort(monkeypatch, OldCompactEngine)
    up = co.quantize_encrypt(_models(n, 3), present=[1, 2, 3])
    assert up.path == "cohort-chain" and co.cipher.engine.log == ["quantize_encrypt_cohort_u32_dev"]
    assert co.cipher.engine.args["quantize_encrypt_cohort_u32_dev"][1] == 1
