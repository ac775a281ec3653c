"""CPU test: plan_cohort's cut_any rule (FlasheCohort(cut="any"), the flashe_*_cohort_cut_runs_* entry points) -- "cut-chain" also for a
short cohort whose present clients form 2 .. 16 runs and for a short batched cohort with 5 - 7 values per element, with the pieces of
cohort_cut_pieces; more than 16 runs, a mixed-float64 cohort, bs 4 and int_bits 64 staged with their reasons; cut_any=False today's plans
-- and the launches FlasheCohort makes on an engine double: the launch that takes the present clients' indices, with a scratch sized from
the library's piece count.  Touches no device and no library."""
import numpy as np
import pytest

from flashe_amd.block import cohort_admission_length, cohort_cut_items, cohort_cut_pieces, compact_cohort_admission_length, plan_cohort
from test_cohort_cut_planner import KEY, CutEngine, StagedEngine, _layer, _models, _W, _ws

CU = 80
N = 700


# ------------------------------------------------------------------------------------------------ the planner
@pytest.mark.parametrize("b", [16, 20, 64, 65, 128])
def test_cut_any_false_is_todays_plan(b):
    adm = cohort_admission_length(CU)
    mixed = _ws(N)
    mixed[1]._weights["a"] = _layer(300, np.float64)
    for n in (1, N, 61706, adm - 1, adm, compact_cohort_admission_length(CU, 16, 16) + 5):
        for kw in ({}, {"mask": "single"}, {"precompute": True}, {"chain": False}, {"batch": True, "element_bits": 4}, {"batch": b > 32},
                   {"compact": b <= 32}, {"compact": b <= 32, "compact_runs": True}, {"precompute": True, "cohort_masks": True}):
            for cut in (False, True):
                for ws, present in ((_ws(n), None), (_ws(n, 4), [0, 1, 3, 4]), (_ws(n, 3), [1, 2, 3]), (_ws(n, 17), list(range(0, 34, 2)))):
                    today = plan_cohort(ws, b, CU, cut=cut, present=present, **kw)
                    assert vars(plan_cohort(ws, b, CU, cut=cut, cut_any=False, present=present, **kw)) == vars(today)
                    if not cut:
                        # cut_any alone widens nothing: it rides on cut
                        assert vars(plan_cohort(ws, b, CU, cut=False, cut_any=True, present=present, **kw)) == vars(today)
                    elif "fill the chip" not in today.reason and today.path != "cut-chain" and "dropped out" not in today.reason:
                        assert vars(plan_cohort(ws, b, CU, cut=True, cut_any=True, present=present, **kw)) == vars(today), (n, kw, present)
    assert vars(plan_cohort(mixed, b, CU, cut=True, cut_any=False)) == vars(plan_cohort(mixed, b, CU, cut=True))


def test_one_run_unbatched_is_the_cut_chain_it_was():
    for kw, b in (({}, 128), ({}, 65), ({"compact": True}, 20), ({"compact": True, "compact_runs": True}, 32)):
        for C, n, present in ((5, N, None), (17, 61706, None), (3, N, [1, 2, 3]), (128, 1, None)):
            old = plan_cohort(_ws(n, C), b, 256, cut=True, present=present, **kw)
            assert old.path == "cut-chain"
            assert vars(plan_cohort(_ws(n, C), b, 256, cut=True, cut_any=True, present=present, **kw)) == vars(old)


def test_a_gapped_short_cohort_plans_the_cut_chain_with_the_pinned_pieces():
    for kw, b in (({}, 128), ({}, 65), ({"compact": True}, 20), ({"compact": True, "compact_runs": True}, 20)):
        old = plan_cohort(_ws(N, 4), b, 256, present=[0, 1, 3, 4], cut=True, **kw)
        assert old.path == "staged-chain" and "2 runs" in old.reason
        p = plan_cohort(_ws(N, 4), b, 256, present=[0, 1, 3, 4], cut=True, cut_any=True, **kw)
        assert (p.path, p.reason, p.parts, p.runs, p.present) == ("cut-chain", "", 2, 2, [0, 1, 3, 4]), kw
        assert (p.n, p.n_elems, p.draw_offsets) == (old.n, old.n_elems, old.draw_offsets)
    # the rule's examples on 256 CUs
    assert plan_cohort(_ws(N, 2), 128, 256, present=[0, 2], cut=True, cut_any=True).parts == 2
    assert plan_cohort(_ws(N, 40), 128, 256, present=[i for i in range(41) if i != 24], cut=True, cut_any=True).parts == 10
    lenet = [i for i in range(100) if i not in (3, 40, 41, 77, 99)]
    assert plan_cohort(_ws(61706, 95), 128, 256, present=lenet, cut=True, cut_any=True).parts == 8
    assert plan_cohort(_ws(61706, 95), 23, 256, present=lenet, cut=True, cut_any=True, compact=True, n_jobs=16).parts == \
        len(cohort_cut_pieces(lenet, cohort_cut_items(61706, 23, 16, True), 256)) - 1
    p = plan_cohort(_ws(N, 16), 128, 256, present=list(range(0, 32, 2)), cut=True, cut_any=True)
    assert (p.path, p.parts, p.runs) == ("cut-chain", 16, 16)
    # seventeen runs: one table holds sixteen chains
    p = plan_cohort(_ws(N, 17), 128, 256, present=list(range(0, 34, 2)), cut=True, cut_any=True)
    assert (p.path, p.parts) == ("staged-chain", 1) and "17 runs" in p.reason and "at most 16 runs" in p.reason
    # from the admission length on the gapped uncut chain runs as before
    adm = cohort_admission_length(CU)
    assert plan_cohort(_ws(adm, 4), 128, CU, present=[0, 1, 3, 4], cut=True, cut_any=True).path == "cohort-chain"


@pytest.mark.parametrize("b,num_clients,bs", [(120, 10, 6), (128, 3, 7), (128, 10, 6), (128, 100, 5)])
def test_a_short_batched_cohort_plans_the_cut_chain(b, num_clients, bs):
    C = min(num_clients, 5)
    old = plan_cohort(_ws(N, C), b, 256, batch=True, num_clients=num_clients, cut=True)
    assert old.path == "staged-chain" and "batched" in old.reason
    p = plan_cohort(_ws(N, C), b, 256, batch=True, num_clients=num_clients, cut=True, cut_any=True)
    n_elems = (300 + bs - 1) // bs + (400 + bs - 1) // bs
    assert (p.path, p.reason, p.n, p.n_elems) == ("cut-chain", "", N, n_elems)
    assert p.parts == len(cohort_cut_pieces(range(C), 2 * ((n_elems + 255) // 256), 256)) - 1 == 1
    if C >= 4:
        g = plan_cohort(_ws(N, 4), b, 256, batch=True, num_clients=num_clients, cut=True, cut_any=True, present=[0, 1, 3, 4])
        assert (g.path, g.parts, g.runs) == ("cut-chain", 2, 2)
    # 100 clients of a LeNet-sized model: the rule counts the batched elements
    if num_clients == 100:
        big = plan_cohort(_ws(61706, 100), b, 256, batch=True, num_clients=100, cut=True, cut_any=True)
        items = cohort_cut_items(61706, b, 16, n_elems=big.n_elems)
        assert big.path == "cut-chain" and items == 2 * ((big.n_elems + 255) // 256) and big.parts == min(16, 4096 // items)
    # from the batched admission length on: the uncut batched chain
    long_ = plan_cohort(_ws(cohort_admission_length(CU) * bs, C), b, CU, batch=True, num_clients=num_clients, cut=True, cut_any=True)
    assert long_.path == "cohort-chain"


def test_what_stays_staged_with_its_reason():
    mixed = _ws(N)
    mixed[1]._weights["a"] = _layer(300, np.float64)
    for ws, kw, b, reason in ((mixed, {}, 128, "a layer is float64 for some clients only"),
                              (mixed, {"batch": True}, 128, "a layer is float64 for some clients only"),
                              (_ws(N), {"batch": True, "element_bits": 4}, 128, "batched job with bs"),
                              (_ws(N), {"batch": True, "element_bits": 29}, 128, "batched job with bs 4"),
                              (_ws(N), {}, 64, "int_bits <= 64"),
                              (_ws(N), {"batch": True}, 64, "int_bits <= 64"),
                              (_ws(N), {"compact": True, "batch": True, "element_bits": 12}, 32, "batched job"),
                              (_ws(N), {"mask": "single"}, 128, "single mask"),
                              (_ws(N, 129), {}, 128, "128 clients")):
        p = plan_cohort(ws, b, CU, cut=True, cut_any=True, **kw)
        assert (p.path, p.parts) == ("staged-chain", 1) and reason in p.reason, (kw, b, p.reason)
    assert plan_cohort(_ws(N, dtype=np.float64), 128, CU, cut=True, cut_any=True, present=[0, 1, 2, 4, 5]).path == "cut-chain"


# ------------------------------------------------------------------------------------------------ the cohort on an engine double
class AnyEngine(CutEngine):
    """An engine with the launches that take the present clients' indices; pieces: what its cohort_cut_pieces answers."""
    pieces = 3

    def cohort_cut_pieces(self, idx, n, n_jobs, compact=False):
        self._rec("cohort_cut_pieces", list(idx), n, n_jobs, compact)
        k = type(self).pieces
        return k, list(range(k)) + [len(idx)] if k else []

    def quantize_encrypt_cohort_cut_runs_dev(self, *a):
        self._rec("quantize_encrypt_cohort_cut_runs_dev", *a)
        return type(self).answer

    def quantize_batch_encrypt_cohort_cut_runs_dev(self, *a):
        self._rec("quantize_batch_encrypt_cohort_cut_runs_dev", *a)
        return type(self).answer

    def combine_unbatch_unquantize_model_dev(self, *a):
        self._rec("combine_unbatch_unquantize_model_dev", *a)


class DecliningAnyEngine(AnyEngine):
    answer = False


class NoPiecesEngine(AnyEngine):
    pieces = 0

    def quantize_encrypt_cohort_cut_runs_dev(self, *a):
        raise AssertionError("the library gave no pieces: nothing to launch")


def _args(b=128, batch=False):
    return {"quantize": {"int_bits": b, "batch": batch, "element_bits": 16, "padding": True, "secure": True}, "precompute": {"enable": False}}


def _cohort(monkeypatch, engine_cls, cut="any", n_local=5, num_clients=5, first_idx=0, batch=False):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheCohort
    monkeypatch.setattr(cm.FlasheCipher, "_engine_cls", engine_cls)
    monkeypatch.setattr(cm, "N_JOBS", 16)
    monkeypatch.setenv("FLASHE_DEVICE_RNG", "0")
    co = FlasheCohort(_args(batch=batch), first_idx=first_idx, n_local=n_local, num_clients=num_clients, prp_seed=KEY, cut=cut)
    co.set_iter_index(4)
    return co


def test_a_gapped_round_is_the_launch_that_takes_the_indices(monkeypatch):
    co = _cohort(monkeypatch, AnyEngine)
    np.random.seed(3)
    up = co.quantize_encrypt(_models(N, 4), present=[0, 1, 3, 4])
    eng = co.cipher.engine
    assert up.path == "cut-chain" and eng.log == ["cohort_cut_pieces", "quantize_encrypt_cohort_cut_runs_dev"] and up.present == [0, 1, 3, 4]
    assert eng.args["cohort_cut_pieces"] == ([0, 1, 3, 4], N, 16, False)
    a = eng.args["quantize_encrypt_cohort_cut_runs_dev"]
    assert a[:4] == (4, [0, 1, 3, 4], N, 16) and len(a[4]) == 2 and len(a[5]) == 4
    mask, scratch = a[-2], a[-1]
    assert mask is not None and scratch.nbytes == 3 * N * 16 * 2                      # three pieces' sums and masks
    m = co.lead._cohort_mask
    assert m[0] == up.partial_sum.ptr and m[2:] == (4, [2, 5], [0, 3]) and len(m[1]) == N      # the telescoped lists
    eng.log.clear()
    co.lead.quantizer.alpha_list = [0.5, 0.5]
    co.lead._decrypt_floats(up.partial_sum, [7, N - 7], None, [2, 5], [0, 3])
    assert eng.log == ["combine_unquantize_model_dev"]
    # a cohort inside a larger federation: the global indices, no mask, half the scratch
    co = _cohort(monkeypatch, AnyEngine, n_local=6, num_clients=12, first_idx=3)
    up = co.quantize_encrypt(_models(N, 4), present=[0, 1, 4, 5])
    a = co.cipher.engine.args["quantize_encrypt_cohort_cut_runs_dev"]
    assert up.path == "cut-chain" and a[1] == [3, 4, 7, 8] and a[-2] is None and a[-1].nbytes == 3 * N * 16 and co.lead._cohort_mask is None
    assert up.present == [3, 4, 7, 8]
    # one run, un-batched: the call cut=True makes
    co = _cohort(monkeypatch, AnyEngine)
    assert co.quantize_encrypt(_models(N, 5)).path == "cut-chain" and co.cipher.engine.log == ["quantize_encrypt_cohort_cut_dev"]


def test_a_batched_round_is_the_batched_cut_launch(monkeypatch):
    bs = 128 // 19                                           # element_bits 16 + ceil(log2 5) = 19 bits a field: 6 values per element
    n_elems = (7 + bs - 1) // bs + (N - 7 + bs - 1) // bs
    for present, idxs, tele in ((None, [0, 1, 2, 3, 4], ([5], [0])), ([0, 2, 3], [0, 2, 3], ([1, 4], [0, 2]))):
        co = _cohort(monkeypatch, AnyEngine, batch=True)
        up = co.quantize_encrypt(_models(N, len(idxs)), present=present)
        eng = co.cipher.engine
        assert up.path == "cut-chain" and eng.log == ["cohort_cut_pieces", "quantize_batch_encrypt_cohort_cut_runs_dev"]
        assert eng.args["cohort_cut_pieces"] == (idxs, n_elems, 16, False)          # the rule counts the batched elements
        a = eng.args["quantize_batch_encrypt_cohort_cut_runs_dev"]
        assert a[:5] == (4, idxs, N, n_elems, 16) and a[8:10] == (16, 19)
        assert a[-2] is not None and a[-1].nbytes == 3 * n_elems * 16 * 2
        m = co.lead._cohort_mask
        assert m[0] == up.partial_sum.ptr and m[2:] == (4,) + tele and len(m[1]) == n_elems and len(up.partial_sum) == n_elems
        eng.log.clear()
        co.lead.quantizer.alpha_list = [0.5, 0.5]
        co.lead._decrypt_floats(up.partial_sum, [7, N - 7], None, *tele)
        assert eng.log == ["combine_unbatch_unquantize_model_dev"]                  # one combine + unbatch pass


def test_cut_values_and_engines_without_the_entry_points(monkeypatch):
    from flashe_amd.block import FlasheCohort
    for bad in ("sometimes", "Any", 2, None, "true"):
        with pytest.raises(ValueError, match="cut"):
            _cohort(monkeypatch, AnyEngine, cut=bad)
    assert FlasheCohort.__init__.__defaults__[-1] is False
    # an engine with the one-run cut launch only: cut="any" behaves as cut=True
    for present, C in ((None, 5), ([0, 1, 3, 4], 4)):
        a, t = _cohort(monkeypatch, CutEngine, cut="any"), _cohort(monkeypatch, CutEngine, cut=True)
        assert vars(a.plan(_models(N, C), present)) == vars(t.plan(_models(N, C), present))
    co = _cohort(monkeypatch, CutEngine, cut="any")
    up = co.quantize_encrypt(_models(N, 4), present=[0, 1, 3, 4])
    assert up.path == "staged-chain" and co.cipher.engine.log == ["quantize_batch_tensors_dev"] * 4 + ["encrypt_batch_sum_dev"]
    # an engine without any cut launch, and cut=True / False on an engine that has them all: today's plans
    assert _cohort(monkeypatch, StagedEngine, cut="any").plan(_models(N, 4), [0, 1, 3, 4]).path == "staged-chain"
    for cut in (True, False):
        p = _cohort(monkeypatch, AnyEngine, cut=cut).plan(_models(N, 4), [0, 1, 3, 4])
        assert p.path == "staged-chain" and ("one run" in p.reason if cut else "fill the chip" in p.reason)
    assert _cohort(monkeypatch, AnyEngine, cut=True, batch=True).plan(_models(N, 5)).path == "staged-chain"


def test_a_declining_library_falls_back_to_the_staged_form(monkeypatch):
    staged = ["quantize_batch_tensors_dev"] * 4 + ["encrypt_batch_sum_dev"]
    co = _cohort(monkeypatch, DecliningAnyEngine)
    up = co.quantize_encrypt(_models(N, 4), present=[0, 1, 3, 4])
    assert up.path == "staged-chain" and co.cipher.engine.log == ["cohort_cut_pieces", "quantize_encrypt_cohort_cut_runs_dev"] + staged
    assert co.lead._cohort_mask is None and co.cipher.engine.args["encrypt_batch_sum_dev"][1] == [0, 1, 3, 4]
    co = _cohort(monkeypatch, NoPiecesEngine)
    up = co.quantize_encrypt(_models(N, 4), present=[0, 1, 3, 4])
    assert up.path == "staged-chain" and co.cipher.engine.log == ["cohort_cut_pieces"] + staged
    co = _cohort(monkeypatch, DecliningAnyEngine, batch=True)
    up = co.quantize_encrypt(_models(N, 5))
    assert up.path == "staged-chain" and co.cipher.engine.log[:2] == ["cohort_cut_pieces", "quantize_batch_encrypt_cohort_cut_runs_dev"]
    assert co.cipher.engine.log[2:] == ["quantize_batch_tensors_dev"] * 5 + ["encrypt_batch_sum_dev"]
    # prefer="staged-chain" never asks
    co = _cohort(monkeypatch, AnyEngine)
    co.prefer = "staged-chain"
    assert co.plan(_models(N, 4), [0, 1, 3, 4]).path == "cut-chain"
    assert co.quantize_encrypt(_models(N, 4), present=[0, 1, 3, 4]).path == "staged-chain" and co.cipher.engine.log == staged
