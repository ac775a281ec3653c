"""GPU, class level: a ONE-LIMB FlasheCohort round in which clients DROPPED OUT (FlasheCohort(one_limb=True).quantize_encrypt(present=...))
against the present clients run one after the other as FlasheClients in one process -- every ciphertext and their sum as uint64 values,
NumPy's generator, alpha_list, shape_dict, the mean / std history and the floats of decrypt_unquantize() against the first present
client's own set_idx_list(present) decrypt, compared as bytes.  int_bits 36 with element_bits 32 (prf_limb_cohort_runs_kernel<3>) for two
rounds, the second normalises, and one round at int_bits 64 (prf_limb_cohort_runs_kernel<2>); five clients of five, at the chip's admission
length plus an odd remainder cut into uneven layers.  `up.path` is asserted everywhere; no mask is kept at these widths, so the decrypt
of the sum is a decrypt launch with the telescoped lists and no combine pass.  The buffers the round allocates are poisoned first."""
import numpy as np
import pytest

from test_gpu_cohort import KEY, _W, _args, _host_models, _poison, _same_state
from test_gpu_cohort_dropout import _Calls
from test_gpu_cohort_limb import _cu_count, _model_sizes, _values_of

pytestmark = pytest.mark.gpu

N_LOCAL = 5
PATTERNS = {
    "one-gap": [0, 1, 3, 4],          # the stream between the runs closes one output and opens none
    "every-other": [0, 2, 4],         # every stream is a run boundary
}


def _sizes(b, tiny=False):
    from flashe_amd.block import compact_cohort_admission_length
    if tiny:
        return [1, 6, 0, 1019, 777]
    return _model_sizes(compact_cohort_admission_length(_cu_count(), b, 16) + 301)


def _make(b, eb):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheClient, FlasheCohort
    cm.N_JOBS = 16
    clients = []
    for c in range(N_LOCAL):
        cl = FlasheClient(_args(b, eb))
        cl.create_cipher(c, N_LOCAL, KEY)
        clients.append(cl)
    co = FlasheCohort(_args(b, eb), first_idx=0, n_local=N_LOCAL, num_clients=N_LOCAL, prp_seed=KEY, one_limb=True)
    assert co.one_limb and hasattr(co.cipher.engine, "quantize_encrypt_cohort_runs_u64_dev")
    return clients, co


def _round(clients, co, present, models, it, normalize, want_path, n):
    """One round of both sides from the same stream position, the decrypt included."""
    here = [clients[p] for p in present]
    mine = [models[p] for p in present]
    for cl in clients:
        cl.set_iter_index(it)
    co.set_iter_index(it)
    np.random.seed(7 + it)
    np.random.random(3)                                       # an odd position in the stream
    state = np.random.get_state()
    want = []
    for cl, m in zip(here, mine):                             # the present clients, one after the other; absent clients draw nothing
        w = cl.quantize_encrypt(_W(dict(m)), device=True, normalize=normalize)
        want.append(w._weights[w.walking_order[0]])
    want_state = np.random.get_state()
    want_sum = here[0].cipher.aggregate(want)
    assert len(want_sum) == n
    eng = co.cipher.engine
    _poison(eng, [8 * n] * (len(present) + 1))
    np.random.set_state(state)
    up = co.quantize_encrypt([_W(dict(m)) for m in mine], normalize=normalize, present=present)
    assert up.path == want_path and up.present == present and len(up.ciphertexts) == len(present)
    assert _same_state(np.random.get_state(), want_state), "the NumPy stream must be left where the sequential steps leave it"
    for v in up.ciphertexts + [up.partial_sum]:
        assert not getattr(v, "compact", False) and v.elem_bytes == 8 and len(v) == n
    for c in range(len(present)):
        assert np.array_equal(_values_of(up.ciphertexts[c]), _values_of(want[c])), (it, present[c])
    assert np.array_equal(_values_of(up.partial_sum), _values_of(want_sum)), it
    assert co.shape_dict == here[0].shape_dict
    assert [float(a).hex() for a in co.quantizer.alpha_list] == [float(a).hex() for a in here[0].quantizer.alpha_list]
    assert co.lead._cohort_mask is None                       # no mask in the one-limb layout
    # the decrypt: the first present client's own, told who uploaded
    here[0].set_idx_list(list(present))
    ref = here[0].decrypt_unquantize(_W({sorted(models[0])[0]: want_sum}), unnormalize=True)
    calls = _Calls(eng)
    try:
        got = co.decrypt_unquantize(unnormalize=True)
    finally:
        calls.restore()
    assert calls.seen and not any(name.startswith("combine") for name in calls.seen), calls.seen
    assert got.walking_order == ref.walking_order
    for k in ref.walking_order:
        assert np.asarray(got._weights[k]).shape == np.asarray(ref._weights[k]).shape
        assert np.asarray(got._weights[k], dtype=np.float64).tobytes() == np.asarray(ref._weights[k], dtype=np.float64).tobytes(), (it, k)
    qa, qb = co.quantizer, here[0].quantizer
    assert [float(x).hex() for x in qa.past_layer_mean_list] == [float(x).hex() for x in qb.past_layer_mean_list]
    assert [float(x).hex() for x in qa.past_layer_std_list] == [float(x).hex() for x in qb.past_layer_std_list]
    for cl in clients:                                        # every client of the federation decrypts the same model: one state
        if cl is not here[0]:
            cl.quantizer.past_layer_mean_list = list(qb.past_layer_mean_list)
            cl.quantizer.past_layer_std_list = list(qb.past_layer_std_list)
    return up


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_a_one_limb_round_with_dropouts_is_the_present_clients_one_after_the_other(pattern):
    present = PATTERNS[pattern]
    sizes = _sizes(36)
    clients, co = _make(36, 32)
    for it in range(2):
        models = _host_models(N_LOCAL, sizes, 100 + it)
        p = co.plan([_W(dict(models[q])) for q in present], present=present)
        assert (p.path, p.runs) == ("cohort-chain", len(present) - 2 if pattern == "one-gap" else len(present))
        _round(clients, co, present, models, it, it == 1, "cohort-chain", sum(sizes))


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_a_one_limb_round_with_dropouts_at_int_bits_64(pattern):
    sizes = _sizes(64)
    clients, co = _make(64, 48)
    _round(clients, co, PATTERNS[pattern], _host_models(N_LOCAL, sizes, 200), 1, False, "cohort-chain", sum(sizes))


def test_the_a_b_switch_runs_a_gapped_one_limb_cohort_staged_with_the_same_values():
    """prefer = "staged-chain" (what the in-process A/B alternates): the gapped indices through the staged form at the chain's length."""
    sizes = _sizes(36)
    clients, co = _make(36, 32)
    co.prefer = "staged-chain"
    models = _host_models(N_LOCAL, sizes, 400)
    _round(clients, co, [0, 1, 3, 4], models, 1, False, "staged-chain", sum(sizes))


def test_a_tiny_gapped_one_limb_model_still_runs_staged():
    sizes = _sizes(36, tiny=True)
    clients, co = _make(36, 32)
    models = _host_models(N_LOCAL, sizes, 300)
    p = co.plan([_W(dict(models[q])) for q in (0, 1, 3, 4)], present=[0, 1, 3, 4])
    assert p.path == "staged-chain" and "fill the chip" in p.reason
    _round(clients, co, [0, 1, 3, 4], models, 2, False, "staged-chain", sum(sizes))
