"""CPU test: plan_cohort(limb_runs=...) -- a ONE-LIMB cohort round (int_bits 33 .. 64) in which clients dropped out, on an engine that has the
gapped one-limb launch (flashe_quantize_encrypt_cohort_runs_u64_dev).  limb_runs=True lets a gapped one-limb cohort through to the 144-stream
rule and the mixed-float64 rule, every other rule speaks as before; the default keyword answers what plan_cohort always answered.  On an
engine double that records calls: FlasheCohort asks limb_runs of the engine, hands the new launch the present clients' cipher indices and
keeps no mask; an engine double with only the one-run launch plans and runs a gapped round as before; a declining answer runs the staged
form; prefer never asks.  Touches no device and no library."""
import numpy as np
import pytest

from flashe_amd.block import cohort_admission_length, compact_cohort_admission_length, plan_cohort
from test_cohort_batch_planner import KEY, _W, _layer
from test_cohort_limb_planner import LimbEngine, _args, _models

CU = 80
WIDTHS = (33, 42, 43, 64)


def _ws(n, C=3, dtype=np.float32):
    head = min(n, 1234)
    return [_W({"a": _layer(head, dtype), "b": _layer(0), "c": _layer(n - head)}) for _ in range(C)]


# ------------------------------------------------------------------------------------------------ limb_runs=False: today's plans
@pytest.mark.parametrize("b", [16, 20, 32, 33, 40, 42, 43, 64, 65, 120, 128])
def test_limb_runs_false_is_the_plan_without_the_keyword(b):
    lengths = (1, cohort_admission_length(CU) - 1, cohort_admission_length(CU), compact_cohort_admission_length(CU, min(b, 64), 16),
               compact_cohort_admission_length(CU, 16, 16) + 5)
    presents = (None, [0, 1, 2], [0, 1, 3], [0, 2, 4], [1, 2, 3], [2, 5, 6])
    kws = ({}, {"one_limb": True}, {"one_limb": True, "mask": "single"}, {"one_limb": True, "cut": True}, {"one_limb": True, "n_jobs": 7},
           {"one_limb": True, "batch": True, "element_bits": 8})
    for n in lengths:
        for present in presents:
            for kw in kws:
                for compact in ((False, True) if b <= 32 else (False,)):
                    ws = _ws(n)
                    a = plan_cohort(ws, b, CU, compact=compact, present=present, **kw)
                    e = plan_cohort(ws, b, CU, compact=compact, present=present, limb_runs=False, **kw)
                    assert vars(a) == vars(e), (b, n, present, kw, compact)
    # and under it a gapped one-limb cohort is staged with the reason plan_cohort always gave
    if 33 <= b <= 64:
        p = plan_cohort(_ws(lengths[-1]), b, CU, one_limb=True, present=[0, 1, 3], limb_runs=False)
        assert p.path == "staged-chain" and "one-limb chain takes one run" in p.reason and "2 runs" in p.reason


@pytest.mark.parametrize("b", [16, 32, 65, 128])
def test_other_widths_and_one_run_are_unaffected_by_the_keyword(b):
    n = compact_cohort_admission_length(CU, 16, 16) + 5
    for present in (None, [0, 1, 3], [1, 2, 3]):
        for kw in ({}, {"one_limb": True}):
            for compact in ((False, True) if b <= 32 else (False,)):
                assert vars(plan_cohort(_ws(n), b, CU, compact=compact, present=present, limb_runs=True, **kw)) == \
                    vars(plan_cohort(_ws(n), b, CU, compact=compact, present=present, **kw)), (b, present, kw, compact)
    # one run, and one_limb=False, plan the same with and without the launch at the one-limb widths too
    for w in WIDTHS:
        for present, kw in ((None, {"one_limb": True}), ([1, 2, 3], {"one_limb": True}), ([0, 1, 3], {})):
            assert vars(plan_cohort(_ws(n), w, CU, present=present, limb_runs=True, **kw)) == vars(plan_cohort(_ws(n), w, CU, present=present, **kw))


# ------------------------------------------------------------------------------------------------ limb_runs=True
@pytest.mark.parametrize("n_jobs", [1, 16])
@pytest.mark.parametrize("b", WIDTHS)
def test_a_gapped_one_limb_cohort_chains_on_an_engine_with_the_launch(b, n_jobs):
    ok = dict(one_limb=True, limb_runs=True, n_jobs=n_jobs)
    adm = compact_cohort_admission_length(CU, b, n_jobs)
    p = plan_cohort(_ws(adm), b, CU, present=[0, 1, 3], **ok)
    assert (p.path, p.reason, p.present, p.runs, p.parts) == ("cohort-chain", "", [0, 1, 3], 2, 1)
    assert p.draw_offsets == [c * adm for c in range(3)]
    # one value below the admission length: the length rule speaks, whatever cut= says
    for cut in ({}, {"cut": True}, {"cut": True, "cut_any": True}):
        short = plan_cohort(_ws(adm - 1), b, CU, present=[0, 1, 3], **ok, **cut)
        assert short.path == "staged-chain" and "fill the chip" in short.reason and short.parts == 1
    # the stream limit decides next: 72 singletons are 144 streams, 73 are 146
    one = _ws(adm, 1)
    for C, chains in ((72, True), (73, False)):
        p = plan_cohort(one * C, b, CU, present=list(range(0, 2 * C, 2)), num_clients=256, **ok)
        assert p.runs == C and (p.path == "cohort-chain") == chains, (C, p.path, p.reason)
    assert p.path == "staged-chain" and "144" in p.reason and "73 runs" in p.reason
    # 128 clients in 16 runs fit, in 17 they do not
    for runs, chains in ((16, True), (17, False)):
        present = [c + min(c // (128 // runs), runs - 1) for c in range(128)]
        p = plan_cohort(one * 128, b, CU, present=present, num_clients=256, **ok)
        assert p.runs == runs and (p.path == "cohort-chain") == chains, (runs, p.path, p.reason)
    # a layer that is float64 for some clients only
    mixed = _ws(adm)
    mixed[1]._weights["a"] = _layer(mixed[1]._weights["a"].shape[0], np.float64)
    p = plan_cohort(mixed, b, CU, present=[0, 1, 3], **ok)
    assert p.path == "staged-chain" and "float64 for some clients only" in p.reason
    assert plan_cohort(_ws(adm, dtype=np.float64), b, CU, present=[0, 1, 3], **ok).path == "cohort-chain"
    # the rules in front of it stay
    assert plan_cohort(_ws(adm), b, CU, present=[0, 1, 3], mask="single", **ok).path == "staged-chain"
    assert plan_cohort(_ws(adm), b, CU, present=[0, 1, 3], batch=True, element_bits=8, **ok).reason == "batched job"
    assert plan_cohort(_ws(adm), b, CU, present=[0, 1, 3], chain=False, **ok).reason == "FLASHE_CHAIN=0"
    assert plan_cohort(_ws(adm), b, CU, present=[0, 1, 3], precompute=True, **ok).path == "per-client"


# ------------------------------------------------------------------------------------------------ the cohort on an engine double
class RunsLimbEngine(LimbEngine):
    def quantize_encrypt_cohort_runs_u64_dev(self, *a):
        self._rec("quantize_encrypt_cohort_runs_u64_dev", *a)
        return type(self).answer


class DecliningRunsLimbEngine(RunsLimbEngine):
    answer = False


NAME, ONE_RUN = "quantize_encrypt_cohort_runs_u64_dev", "quantize_encrypt_cohort_u64_dev"
STAGED = ["quantize_batch_tensors_dev"] * 3 + ["encrypt_batch_sum_dev"]


def _cohort(monkeypatch, engine_cls, b=36, first_idx=0, n_local=5, num_clients=5, **kw):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheCohort
    monkeypatch.setattr(cm.FlasheCipher, "_engine_cls", engine_cls)
    monkeypatch.setattr(cm, "N_JOBS", 16)
    monkeypatch.setenv("FLASHE_DEVICE_RNG", "0")
    co = FlasheCohort(_args(b), first_idx=first_idx, n_local=n_local, num_clients=num_clients, prp_seed=KEY, one_limb=True, **kw)
    co.set_iter_index(4)
    return co


@pytest.mark.parametrize("b", [36, 64])
def test_the_cohort_hands_the_runs_launch_the_present_indices_and_keeps_no_mask(monkeypatch, b):
    n = compact_cohort_admission_length(RunsLimbEngine.cu_count, b, 16) + 9
    co = _cohort(monkeypatch, RunsLimbEngine, b=b, first_idx=10, n_local=5, num_clients=20)
    ws = _models(n, 4)
    p = co.plan(ws, present=[0, 1, 3, 4])
    assert co.one_limb and (p.path, p.runs) == ("cohort-chain", 2)
    np.random.seed(3)
    up = co.quantize_encrypt(ws, present=[0, 1, 3, 4])
    eng = co.cipher.engine
    assert up.path == "cohort-chain" and eng.log == [NAME] and up.present == [10, 11, 13, 14] and len(up.ciphertexts) == 4
    a = eng.args[NAME]
    assert a[:4] == (4, [10, 11, 13, 14], n, 16) and len(a[4]) == 2 and len(a[5]) == 4 and a[7] == 32      # iter, idx, n, n_jobs, rows, sources, element_bits
    assert len(a) == 11 and len(a[9]) == 4 and co.lead._cohort_mask is None                             # ... draws, ciphertexts, sum: no mask argument
    for v in up.ciphertexts + [up.partial_sum]:
        assert len(v) == n and v.elem_bytes == 8 and not getattr(v, "compact", False)
    # the whole federation: still no mask, and never the cut launch
    co = _cohort(monkeypatch, RunsLimbEngine, b=b, cut="any")
    up = co.quantize_encrypt(_models(n, 3), present=[0, 2, 4])
    assert co.cipher.engine.log == [NAME] and co.cipher.engine.args[NAME][1] == [0, 2, 4] and co.lead._cohort_mask is None and up.path == "cohort-chain"
    # present=None is the call it always was
    co = _cohort(monkeypatch, RunsLimbEngine, b=b)
    up = co.quantize_encrypt(_models(n, 5))
    assert co.cipher.engine.log == [ONE_RUN] and co.cipher.engine.args[ONE_RUN][1] == 0 and up.path == "cohort-chain"


def test_an_engine_with_only_the_one_run_launch_stages_a_gapped_round(monkeypatch):
    n = compact_cohort_admission_length(LimbEngine.cu_count, 36, 16) + 9
    co = _cohort(monkeypatch, LimbEngine)
    ws = _models(n, 3)
    p = co.plan(ws, present=[0, 1, 3])
    assert p.path == "staged-chain" and "one-limb chain takes one run" in p.reason
    up = co.quantize_encrypt(ws, present=[0, 1, 3])
    assert up.path == "staged-chain" and co.cipher.engine.log == STAGED
    # one run given by `present`: the one-run launch with the first index
    co = _cohort(monkeypatch, LimbEngine)
    up = co.quantize_encrypt(_models(n, 3), present=[1, 2, 3])
    assert up.path == "cohort-chain" and co.cipher.engine.log == [ONE_RUN] and co.cipher.engine.args[ONE_RUN][1] == 1


def test_a_gapped_launch_the_library_declines_runs_the_staged_chain(monkeypatch):
    n = compact_cohort_admission_length(LimbEngine.cu_count, 36, 16) + 9
    co = _cohort(monkeypatch, DecliningRunsLimbEngine)
    up = co.quantize_encrypt(_models(n, 3), present=[0, 1, 3])
    assert up.path == "staged-chain" and co.cipher.engine.log == [NAME] + STAGED
    # a tiny gapped model never asks
    co = _cohort(monkeypatch, RunsLimbEngine)
    up = co.quantize_encrypt(_models(100, 3), present=[0, 1, 3])
    assert up.path == "staged-chain" and co.cipher.engine.log == STAGED


@pytest.mark.parametrize("prefer", ["staged-chain", "per-client"])
def test_prefer_never_asks_the_launch(monkeypatch, prefer):
    n = compact_cohort_admission_length(LimbEngine.cu_count, 36, 16) + 9
    co = _cohort(monkeypatch, RunsLimbEngine)
    co.prefer = prefer
    assert co._choose_path(co.plan(_models(n, 3), present=[0, 1, 3]), [[(None, 0, np.float32)] * 2] * 3) == prefer
    co = _cohort(monkeypatch, RunsLimbEngine)
    co.prefer = "staged-chain"
    up = co.quantize_encrypt(_models(n, 3), present=[0, 1, 3])
    assert up.path == "staged-chain" and co.cipher.engine.log == STAGED
