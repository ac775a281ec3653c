"""CPU test: plan_cohort's rule for BATCHED jobs at int_bits > 64 (flashe_quantize_batch_encrypt_cohort_dev: the chained launch packs 5, 6
or 7 values per element and counts its admission length in batched elements), every other batched shape on the staged form with a reason
that names the cause, and -- on an engine double that records calls -- FlasheCohort's fallback when the library declines and
_CohortLead's choice between the combine pass and the decrypt launch.  Touches no device and no library."""
import numpy as np
import pytest

from flashe_amd.block import cohort_admission_length, plan_cohort

KEY = bytes(range(32))


class _W:
    def __init__(self, layers):
        self.walking_order = sorted(layers)
        self._weights = dict(layers)


def _layer(n, dtype=np.float32):
    return np.broadcast_to(np.zeros((), dtype), (n,))          # (a shape and a dtype: the planner reads nothing else)


def _cohort(n, C=10, dtype=np.float32):
    """One layer of n values: ceil(n / bs) batched elements."""
    return [_W({"w": _layer(n, dtype)}) for _ in range(C)]


def _plan(ws, cu, int_bits=120, num_clients=10, **kw):
    args = dict(element_bits=16, batch=True, mask="double", num_clients=num_clients)
    args.update(kw)
    return plan_cohort(ws, int_bits, cu, **args)


@pytest.mark.parametrize("cu", [256, 80])
def test_a_batched_job_chains_from_the_admission_length_in_elements(cu):
    adm = cohort_admission_length(cu)
    p = _plan(_cohort(6 * adm + 5), cu)
    assert (p.path, p.reason) == ("cohort-chain", "")
    assert p.n == 6 * adm + 5 and p.n_elems == adm + 1 and p.draw_offsets == [c * p.n for c in range(10)]
    at = _plan(_cohort(6 * adm), cu)
    assert at.n_elems == adm and at.path == "cohort-chain"
    below = _plan(_cohort(6 * (adm - 1)), cu)                    # one element below the admission length
    assert below.n_elems == adm - 1 and below.path == "staged-chain" and "fill the chip" in below.reason
    # every layer is padded to whole elements on its own: the count is per layer
    ws = [_W({"a": _layer(1), "b": _layer(0), "c": _layer(6 * (adm - 2) + 1)}) for _ in range(10)]
    assert _plan(ws, cu).n_elems == adm and _plan(ws, cu).path == "cohort-chain"


@pytest.mark.parametrize("cu", [256, 80])
@pytest.mark.parametrize("int_bits, num_clients, bs", [(120, 10, 6), (128, 3, 7), (120, 20, 5), (128, 10, 6)])
def test_the_batch_sizes_of_the_shipped_jobs_chain(cu, int_bits, num_clients, bs):
    adm = cohort_admission_length(cu)
    p = _plan(_cohort(bs * adm, C=2), cu, int_bits=int_bits, num_clients=num_clients)
    assert (p.n_elems, p.path) == (adm, "cohort-chain")
    p = _plan(_cohort(bs * adm - bs, C=2), cu, int_bits=int_bits, num_clients=num_clients)
    assert (p.n_elems, p.path) == (adm - 1, "staged-chain")


@pytest.mark.parametrize("cu", [256, 80])
def test_other_batch_sizes_are_staged_with_a_reason_that_names_bs(cu):
    adm = cohort_admission_length(cu)
    for int_bits, num_clients, bs in ((120, 10, 10), (128, 10, 10), (128, 2, 14)):
        p = _plan(_cohort(bs * adm + 3, C=2), cu, int_bits=int_bits, num_clients=num_clients, element_bits=8)
        assert p.n_elems == adm + 1 and p.path == "staged-chain" and f"bs {bs}" in p.reason, (int_bits, num_clients, p.reason)
    p = _plan(_cohort(8 * adm, C=2), cu, int_bits=128, num_clients=2, element_bits=15)       # bs 8, one past the compiled sizes
    assert p.path == "staged-chain" and "bs 8" in p.reason
    p = _plan(_cohort(4 * adm, C=2), cu, int_bits=120, num_clients=600)                       # bs 4, one below them
    assert p.path == "staged-chain" and "bs 4" in p.reason


@pytest.mark.parametrize("cu", [256, 80])
def test_the_other_rules_are_those_of_the_unbatched_table(cu):
    n = 6 * cohort_admission_length(cu) + 5
    ws = _cohort(n, C=3)
    assert _plan(ws, cu).path == "cohort-chain"
    p = _plan(ws, cu, mask="single")
    assert p.path == "staged-chain" and "single mask" in p.reason
    p = _plan(ws, cu, chain=False)
    assert (p.path, p.reason) == ("staged-chain", "FLASHE_CHAIN=0")
    p = _plan(ws, cu, precompute=True)
    assert p.path == "per-client" and "precomputed" in p.reason
    assert _plan(ws, cu, mask="dynamic").path == "per-client"
    p = _plan(ws, cu, int_bits=64, num_clients=4)
    assert (p.path, p.reason) == ("staged-chain", "int_bits <= 64")
    one = _cohort(n, C=1)
    assert _plan(one * 128, cu, num_clients=128, int_bits=128).path == "cohort-chain"         # (16 + 7 bits: bs 5)
    p = _plan(one * 129, cu, num_clients=129, int_bits=128)                                   # (16 + 8 bits: bs 5)
    assert p.path == "staged-chain" and "128 clients" in p.reason
    mixed = _cohort(n, C=3)
    mixed[1]._weights["w"] = _layer(n, np.float64)
    p = _plan(mixed, cu)
    assert p.path == "staged-chain" and "float64 for some clients only" in p.reason
    assert _plan(_cohort(n, C=3, dtype=np.float64), cu).path == "cohort-chain"
    # the compact layout keeps its answer for batched jobs
    p = plan_cohort(ws, 32, cu, element_bits=12, batch=True, compact=True, n_jobs=16)
    assert (p.path, p.reason) == ("staged-chain", "batched job")


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
    """What FlasheCohort.quantize_encrypt and _CohortLead._decrypt_floats call, recorded by name; nothing is computed."""
    answer = True            # what quantize_batch_encrypt_cohort_dev returns
    limbs, cu_count, device = 2, 2, 0

    def __init__(self, key, int_bits, device=0, stream=None):
        self.int_bits, self._next, self.log, self.args = int_bits, 1 << 20, [], {}

    def set_key(self, key):
        pass

    def alloc(self, nbytes):
        return _Buf(self, nbytes)

    def alloc_vec(self, n, limbs=None):
        return _Buf(self, max(8 * n * (limbs or self.limbs), 16))

    def hold(self, keep):
        pass

    def quantize_encrypt_model_dev(self, *a):
        raise AssertionError("not a call of the cohort")

    def _rec(self, name, *a):
        self.log.append(name)
        self.args[name] = a

    def quantize_batch_encrypt_cohort_dev(self, *a):
        self._rec("quantize_batch_encrypt_cohort_dev", *a)
        return type(self).answer

    def quantize_encrypt_cohort_dev(self, *a):
        raise AssertionError("the un-batched entry point for a batched job")

    def quantize_batch_tensors_dev(self, *a):
        self._rec("quantize_batch_tensors_dev", *a)

    def encrypt_batch_sum_dev(self, *a):
        self._rec("encrypt_batch_sum_dev", *a)

    def decrypt_dev(self, *a):
        self._rec("decrypt_dev", *a)

    def unbatch_unquantize_model_dev(self, *a):
        self._rec("unbatch_unquantize_model_dev", *a)

    def combine_unbatch_unquantize_model_dev(self, *a):
        self._rec("combine_unbatch_unquantize_model_dev", *a)


class DecliningEngine(RecordingEngine):
    answer = False


def _args(b):
    return {"quantize": {"int_bits": b, "batch": True, "element_bits": 16, "padding": True, "secure": True}, "precompute": {"enable": False}}


def _upload(monkeypatch, engine_cls, prefer=None, n_local=3, num_clients=3, extra=5):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheCohort
    monkeypatch.setattr(cm.FlasheCipher, "_engine_cls", engine_cls)
    monkeypatch.setattr(cm, "N_JOBS", 16)
    monkeypatch.setenv("FLASHE_DEVICE_RNG", "0")
    co = FlasheCohort(_args(120), first_idx=0, n_local=n_local, num_clients=num_clients, prp_seed=KEY)
    co.prefer = prefer
    co.set_iter_index(4)
    adm = cohort_admission_length(engine_cls.cu_count)
    sizes = [7, 0, 6 * (adm - 2) + extra]                      # 2 + 0 + (adm - 2 + 1) elements at bs 6
    ws = [_W({f"l{i}": np.zeros(s, np.float32) for i, s in enumerate(sizes)}) for _ in range(n_local)]
    np.random.seed(3)
    up = co.quantize_encrypt(ws)
    return co, up, sizes, adm + 1


def test_the_cohort_calls_the_batched_launch_and_falls_back_when_it_declines(monkeypatch):
    co, up, sizes, n_elems = _upload(monkeypatch, RecordingEngine)
    eng = co.cipher.engine
    assert up.path == "cohort-chain" and eng.log == ["quantize_batch_encrypt_cohort_dev"]
    a = eng.args["quantize_batch_encrypt_cohort_dev"]
    assert a[:5] == (4, 0, sum(sizes), n_elems, 16) and a[8:10] == (16, 18)            # iter, first_idx, n_values, n_elems, n_jobs .. bits
    assert [r[0] for r in a[5]] == [0, 7, 7] and len(a[6]) == 3 and a[13] is not None    # the shared rows, one source row per client, a mask
    assert co.lead._cohort_mask is not None and len(co.lead._cohort_mask[1]) == n_elems
    assert co.shape_dict == {"l0": (2,), "l1": (0,), "l2": (n_elems - 2,)} and co.quantizer.shape_list == [(7,), (0,), (sizes[2],)]
    assert all(len(v) == n_elems for v in up.ciphertexts) and len(up.partial_sum) == n_elems

    staged = ["quantize_batch_tensors_dev"] * 3 + ["encrypt_batch_sum_dev"]
    co, up, sizes, n_elems = _upload(monkeypatch, DecliningEngine)
    assert up.path == "staged-chain" and co.cipher.engine.log == ["quantize_batch_encrypt_cohort_dev"] + staged
    assert co.lead._cohort_mask is None
    assert co.shape_dict == {"l0": (2,), "l1": (0,), "l2": (n_elems - 2,)}
    # the A/B switch and a model one element short never ask
    co, up, _s, _n = _upload(monkeypatch, RecordingEngine, prefer="staged-chain")
    assert up.path == "staged-chain" and co.cipher.engine.log == staged
    co, up, _s, _n = _upload(monkeypatch, RecordingEngine, extra=-6)            # (adm - 1 elements)
    assert up.path == "staged-chain" and co.cipher.engine.log == staged
    # a cohort inside a larger federation chains (field_bits 16 + 3: bs 6) and keeps no mask
    co, up, _s, _n = _upload(monkeypatch, RecordingEngine, n_local=3, num_clients=5)
    a = co.cipher.engine.args["quantize_batch_encrypt_cohort_dev"]
    assert up.path == "cohort-chain" and a[9] == 19 and a[13] is None and co.lead._cohort_mask is None


def test_the_lead_takes_the_combine_pass_only_with_a_matching_mask(monkeypatch):
    from flashe_amd.engine import DeviceVector
    co, up, sizes, n_elems = _upload(monkeypatch, RecordingEngine)
    ld, eng = co.lead, co.cipher.engine
    ld.quantizer.alpha_list = [0.5, 0.5, 0.5]

    def run(dv, add, minus, it=4):
        eng.log.clear()
        ld.cipher.set_iter_index(it)
        ld._decrypt_floats(dv, sizes, None, add, minus)
        return list(eng.log)

    assert run(up.partial_sum, [3], [0]) == ["combine_unbatch_unquantize_model_dev"]
    a = eng.args["combine_unbatch_unquantize_model_dev"]
    assert a[1:4] == (16, 18, 3) and a[4] is up.partial_sum.buf and a[5] is ld._cohort_mask[1].buf and a[6] is None and a[7] == n_elems
    assert [l[0] for l in a[0]] == sizes
    launch = ["decrypt_dev", "unbatch_unquantize_model_dev"]
    assert run(DeviceVector(eng, n_elems), [3], [0]) == launch                # another vector
    assert run(up.partial_sum, [3], [0], it=5) == launch                      # another iteration
    assert run(up.partial_sum, [2], [0]) == launch                            # other clients
    assert run(up.partial_sum, [3], [1]) == launch
    with pytest.raises(ValueError):
        ld._decrypt_floats(up.partial_sum, [sizes[0], sizes[1], sizes[2] + 6], None, [3], [0])
    ld._cohort_mask = None
    assert run(up.partial_sum, [3], [0]) == launch                            # no mask
