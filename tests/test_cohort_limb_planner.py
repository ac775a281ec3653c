"""CPU test: plan_cohort's one_limb=True rule (FlasheCohort(one_limb=True), flashe_quantize_encrypt_cohort_u64_dev) -- the chained launch at
int_bits 33 .. 64 in the one-limb layout from exactly the admission length of the summed chain on, whatever the chunking, every other
shape on the fallback it takes today with the reason it has today -- and one_limb=False, the default, unchanged on a grid of shapes.  On
an engine double that records calls: the cohort hands the launch the first cipher index and keeps no mask, falls back when the library
declines, behaves as one_limb=False on an engine without the entry point, and refuses a job outside int_bits 33 .. 64.  Touches no
device and no library."""
import numpy as np
import pytest

from flashe_amd.block import cohort_admission_length, compact_cohort_admission_length, compact_cohort_blocks, plan_cohort
from test_cohort_batch_planner import KEY, RecordingEngine, _W, _layer

CU = 80
WIDTHS = (33, 42, 43, 64)


def _ws(n, C=3, dtype=np.float32):
    head = min(n, 1234)
    return [_W({"a": _layer(head, dtype), "b": _layer(0), "c": _layer(n - head)}) for _ in range(C)]


# ------------------------------------------------------------------------------------------------ one_limb=False: today's plans
@pytest.mark.parametrize("b", [16, 20, 32, 33, 40, 42, 43, 64, 65, 120, 128])
def test_one_limb_false_is_the_plan_without_the_keyword(b):
    lengths = (1, cohort_admission_length(CU) - 1, cohort_admission_length(CU), compact_cohort_admission_length(CU, min(b, 64), 16),
               compact_cohort_admission_length(CU, 16, 16) + 5)
    kws = ({}, {"mask": "single"}, {"precompute": True}, {"chain": False}, {"batch": True, "element_bits": 12}, {"batch": True, "element_bits": 4},
           {"present": [0, 2]}, {"present": [1, 2]}, {"cut": True}, {"cut": True, "cut_any": True, "present": [0, 2]}, {"n_jobs": 7},
           {"cohort_masks": True, "precompute": True})
    for n in lengths:
        for kw in kws:
            for compact in ((False, True) if b <= 32 else (False,)):
                ws = _ws(n, C=2 if "present" in kw else 3)
                a = plan_cohort(ws, b, CU, compact=compact, **kw)
                e = plan_cohort(ws, b, CU, compact=compact, one_limb=False, **kw)
                assert vars(a) == vars(e), (b, n, kw, compact)
                if not kw and not compact and b <= 64:
                    assert (a.path, a.reason) == ("staged-chain", "int_bits <= 64")


@pytest.mark.parametrize("b", [16, 32, 65, 128])
def test_other_widths_are_unaffected_by_the_keyword(b):
    for n in (cohort_admission_length(CU) - 1, cohort_admission_length(CU), compact_cohort_admission_length(CU, 16, 16) + 5):
        for kw in ({}, {"mask": "single"}, {"chain": False}, {"present": [0, 2]}, {"cut": True}):
            for compact in ((False, True) if b <= 32 else (False,)):
                ws = _ws(n, C=2 if "present" in kw else 3)
                assert vars(plan_cohort(ws, b, CU, compact=compact, one_limb=True, **kw)) == vars(plan_cohort(ws, b, CU, compact=compact, **kw)), (b, n, kw)
    assert plan_cohort(_ws(10 ** 6), 32, CU, one_limb=True).reason == "int_bits <= 64"


# ------------------------------------------------------------------------------------------------ one_limb=True
@pytest.mark.parametrize("n_jobs", [1, 7, 16])
@pytest.mark.parametrize("b", WIDTHS)
def test_the_one_limb_chain_from_the_admission_length_on(b, n_jobs):
    need = 2 * 128 * 16 * CU
    n = compact_cohort_admission_length(CU, b, n_jobs)
    assert compact_cohort_blocks(n, b, n_jobs) >= need > compact_cohort_blocks(n - 1, b, n_jobs)
    at = plan_cohort(_ws(n), b, CU, one_limb=True, n_jobs=n_jobs)
    assert (at.path, at.reason, at.n, at.n_elems, at.parts) == ("cohort-chain", "", n, n, 1)
    below = plan_cohort(_ws(n - 1), b, CU, one_limb=True, n_jobs=n_jobs)
    assert (below.path, below.reason) == ("staged-chain", "the vector does not fill the chip uncut")
    # (the cut launch does not take these widths: a short one-limb cohort stays staged whatever cut= says)
    for cut in ({"cut": True}, {"cut": True, "cut_any": True}):
        p = plan_cohort(_ws(n - 1), b, CU, one_limb=True, n_jobs=n_jobs, **cut)
        assert (p.path, p.reason, p.parts) == ("staged-chain", "the vector does not fill the chip uncut", 1)


@pytest.mark.parametrize("n_jobs", [1, 7, 16])
@pytest.mark.parametrize("b", WIDTHS)
def test_every_fallback_rule_gives_its_reason(b, n_jobs):
    ok = dict(one_limb=True, n_jobs=n_jobs)
    n = compact_cohort_admission_length(CU, b, n_jobs) + 1000
    assert plan_cohort(_ws(n), b, CU, **ok).path == "cohort-chain"
    # the reasons are the ones the planner has today
    today = lambda **kw: plan_cohort(_ws(n), 20, CU, compact=True, n_jobs=n_jobs, **kw)      # noqa: E731
    p = plan_cohort(_ws(n), b, CU, mask="single", **ok)
    assert (p.path, p.reason) == ("staged-chain", today(mask="single").reason) and "single mask" in p.reason
    p = plan_cohort(_ws(n), b, CU, batch=True, element_bits=8, **ok)
    assert (p.path, p.reason) == ("staged-chain", "batched job")
    p = plan_cohort(_ws(n, C=129), b, CU, **ok)
    assert (p.path, p.reason) == ("staged-chain", "more than 128 clients")
    assert plan_cohort(_ws(n, C=128), b, CU, **ok).path == "cohort-chain"
    p = plan_cohort(_ws(n), b, CU, chain=False, **ok)
    assert (p.path, p.reason) == ("staged-chain", "FLASHE_CHAIN=0")
    p = plan_cohort(_ws(n), b, CU, precompute=True, **ok)
    assert p.path == "per-client" and "precomputed" in p.reason
    # several runs: staged, and the reason names the one-limb chain; one run given by `present` chains
    p = plan_cohort(_ws(n, C=3), b, CU, present=[0, 1, 3], **ok)
    assert p.path == "staged-chain" and "one-limb chain" in p.reason and "2 runs" in p.reason
    assert plan_cohort(_ws(n, C=3), b, CU, present=[1, 2, 3], **ok).path == "cohort-chain"
    mixed = _ws(n)
    mixed[1]._weights["a"] = _layer(mixed[1]._weights["a"].shape[0], np.float64)
    p = plan_cohort(mixed, b, CU, **ok)
    assert p.path == "staged-chain" and "float64 for some clients only" in p.reason
    assert plan_cohort(_ws(n, dtype=np.float64), b, CU, **ok).path == "cohort-chain"            # (float64 for all: a shared row)


def test_a_vector_of_two_to_the_thirty_two_values_does_not_chain():
    class _Huge(_W):
        pass
    w = [_Huge({"a": np.broadcast_to(np.zeros((), np.float32), (2 ** 32,))}) for _ in range(2)]
    p = plan_cohort(w, 64, 2, one_limb=True, n_jobs=16)
    assert (p.path, p.reason) == ("staged-chain", "the vector does not fill the chip uncut")
    w = [_Huge({"a": np.broadcast_to(np.zeros((), np.float32), (2 ** 32 - 1,))}) for _ in range(2)]
    assert plan_cohort(w, 64, 2, one_limb=True, n_jobs=16).path == "cohort-chain"


# ------------------------------------------------------------------------------------------------ the cohort on an engine double
class StagedEngine(RecordingEngine):
    """A one-limb engine from before the entry point."""
    limbs, cu_count = 1, 2

    def quantize_batch_tensors_dev(self, *a):
        self._rec("quantize_batch_tensors_dev", *a)

    def encrypt_batch_sum_dev(self, *a):
        self._rec("encrypt_batch_sum_dev", *a)


class LimbEngine(StagedEngine):
    def quantize_encrypt_cohort_u64_dev(self, *a):
        self._rec("quantize_encrypt_cohort_u64_dev", *a)
        return type(self).answer


class DecliningLimbEngine(LimbEngine):
    answer = False


def _args(b, eb=32):
    return {"quantize": {"int_bits": b, "batch": False, "element_bits": eb, "padding": True, "secure": True}, "precompute": {"enable": False}}


def _cohort(monkeypatch, engine_cls, b=36, first_idx=0, n_local=3, num_clients=3, **kw):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheCohort
    monkeypatch.setattr(cm.FlasheCipher, "_engine_cls", engine_cls)
    monkeypatch.setattr(cm, "N_JOBS", 16)
    monkeypatch.setenv("FLASHE_DEVICE_RNG", "0")
    co = FlasheCohort(_args(b), first_idx=first_idx, n_local=n_local, num_clients=num_clients, prp_seed=KEY, **kw)
    co.set_iter_index(4)
    return co


def _models(n_values, C):
    return [_W({"a": np.zeros(7, np.float32), "b": np.zeros(n_values - 7, np.float32)}) for _ in range(C)]


NAME = "quantize_encrypt_cohort_u64_dev"


def test_the_cohort_hands_the_launch_the_first_index_and_keeps_no_mask(monkeypatch):
    n = compact_cohort_admission_length(LimbEngine.cu_count, 36, 16) + 9
    co = _cohort(monkeypatch, LimbEngine, first_idx=5, n_local=3, num_clients=9, one_limb=True)
    assert co.one_limb and co.plan(_models(n, 3)).path == "cohort-chain"
    np.random.seed(3)
    up = co.quantize_encrypt(_models(n, 3))
    eng = co.cipher.engine
    assert up.path == "cohort-chain" and eng.log == [NAME] and len(up.ciphertexts) == 3
    a = eng.args[NAME]
    assert a[:4] == (4, 5, n, 16) and len(a[4]) == 2 and len(a[5]) == 3 and a[7] == 32          # iter, first_idx, n, n_jobs, rows, sources, element_bits
    assert len(a) == 11 and len(a[9]) == 3                                                        # ... draws, ciphertexts, sum: no mask argument
    for v in up.ciphertexts + [up.partial_sum]:
        assert len(v) == n and v.elem_bytes == 8 and not getattr(v, "compact", False)
    # the whole federation: still no mask kept
    co = _cohort(monkeypatch, LimbEngine, one_limb=True)
    up = co.quantize_encrypt(_models(n, 3))
    assert up.path == "cohort-chain" and co.lead._cohort_mask is None
    # one run given by `present`: its first client's index
    co = _cohort(monkeypatch, LimbEngine, n_local=5, num_clients=5, one_limb=True)
    up = co.quantize_encrypt(_models(n, 3), present=[1, 2, 3])
    assert up.path == "cohort-chain" and co.cipher.engine.args[NAME][1] == 1
    # several runs: staged
    co = _cohort(monkeypatch, LimbEngine, n_local=5, num_clients=5, one_limb=True)
    up = co.quantize_encrypt(_models(n, 3), present=[0, 1, 3])
    assert up.path == "staged-chain" and NAME not in co.cipher.engine.log
    # one value below admission: staged
    co = _cohort(monkeypatch, LimbEngine, one_limb=True)
    short = compact_cohort_admission_length(LimbEngine.cu_count, 36, 16) - 1
    up = co.quantize_encrypt(_models(short, 3))
    assert up.path == "staged-chain" and co.cipher.engine.log == ["quantize_batch_tensors_dev"] * 3 + ["encrypt_batch_sum_dev"]


@pytest.mark.parametrize("prefer", ["staged-chain", "per-client"])
def test_prefer_never_asks_the_launch(monkeypatch, prefer):
    n = compact_cohort_admission_length(LimbEngine.cu_count, 36, 16) + 9
    co = _cohort(monkeypatch, LimbEngine, one_limb=True)
    co.prefer = prefer
    assert co._choose_path(co.plan(_models(n, 3)), [[(None, 0, np.float32)] * 2] * 3) == prefer


def test_a_launch_the_library_declines_runs_the_staged_chain(monkeypatch):
    n = compact_cohort_admission_length(LimbEngine.cu_count, 36, 16) + 9
    co = _cohort(monkeypatch, DecliningLimbEngine, one_limb=True)
    up = co.quantize_encrypt(_models(n, 3))
    assert up.path == "staged-chain"
    assert co.cipher.engine.log == [NAME] + ["quantize_batch_tensors_dev"] * 3 + ["encrypt_batch_sum_dev"]


def test_the_default_and_an_engine_without_the_entry_point_run_as_before(monkeypatch):
    n = compact_cohort_admission_length(LimbEngine.cu_count, 36, 16) + 9
    for cls, kw in ((LimbEngine, {}), (LimbEngine, {"one_limb": False}), (StagedEngine, {"one_limb": True})):
        co = _cohort(monkeypatch, cls, **kw)
        assert not co.one_limb
        p = co.plan(_models(n, 3))
        assert (p.path, p.reason) == ("staged-chain", "int_bits <= 64")
        up = co.quantize_encrypt(_models(n, 3))
        assert up.path == "staged-chain" and co.cipher.engine.log == ["quantize_batch_tensors_dev"] * 3 + ["encrypt_batch_sum_dev"]


@pytest.mark.parametrize("b", [20, 32, 65, 128])
def test_one_limb_needs_int_bits_33_to_64(monkeypatch, b):
    with pytest.raises(ValueError, match="int_bits"):
        _cohort(monkeypatch, LimbEngine, b=b, one_limb=True)
    for ok in (33, 64):
        assert _cohort(monkeypatch, LimbEngine, b=ok, one_limb=True).one_limb
