"""GPU, class level: a FlasheCohort round in which clients DROPPED OUT (quantize_encrypt(present=...)) against the present clients run
one after the other as FlasheClients in one process -- every ciphertext, their sum, NumPy's generator, alpha_list, shape_dict and the
floats of decrypt_unquantize() against the first present client's own set_idx_list(present) decrypt, compared as bytes, for two rounds
(the second normalises).  int_bits 128 un-batched (prf_chain_cohort_runs_kernel) and int_bits 120 batched with element_bits 16, six values
per element (prf_chain_cohort_batch_runs_kernel<1024, 6>), five clients of five, at the chip's admission length plus an odd remainder cut
into uneven layers.  `up.path` is asserted everywhere and the decrypt must take the mask the launch wrote: one combine pass, no PRF
launch.  The buffers the round allocates are poisoned first."""
import numpy as np
import pytest

from test_gpu_cohort import KEY, _W, _args, _cu_count, _host_models, _model_sizes, _poison, _same_state

pytestmark = pytest.mark.gpu

N_LOCAL = 5
# the present set and what it exercises
PATTERNS = {
    "one-gap": [0, 1, 3, 4],          # the stream between the runs closes one output and opens none
    "both-ends": [1, 2],              # gaps at both ends: one run that does not start at the cohort's first client
    "singletons": [0, 4],             # the interior streams 2 and 3 are skipped
    "every-other": [0, 2, 4],         # every stream is a run boundary
    "everyone": [0, 1, 2, 3, 4],      # one run: the kernels and the bytes of a call without `present`
}
SETTINGS = {"128": (128, False), "120-batched": (120, True)}


def _bs(b, batch):
    return b // (16 + int(np.ceil(np.log2(N_LOCAL)))) if batch else 1


def _sizes(b, batch, tiny=False):
    from flashe_amd.block import cohort_admission_length
    if tiny:
        return [1, 6, 0, 1019, 777]
    # (an odd remainder past the admission length; a batched layer is padded to whole elements on its own, so at least that many elements)
    return _model_sizes(_bs(b, batch) * (cohort_admission_length(_cu_count()) + 300))


def _make(b, batch, precompute_params=None):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheClient, FlasheCohort
    cm.N_JOBS = 16
    args = _args(b, 16, batch)
    if precompute_params is not None:
        args["precompute"] = {"enable": True, "num_params": precompute_params}
    clients = []
    for c in range(N_LOCAL):
        cl = FlasheClient(args)
        cl.create_cipher(c, N_LOCAL, KEY)
        clients.append(cl)
    return clients, FlasheCohort(args, first_idx=0, n_local=N_LOCAL, num_clients=N_LOCAL, prp_seed=KEY)


class _Calls:
    """Counts the engine's decrypt back ends while it is installed."""
    NAMES = ("combine_unquantize_model_dev", "combine_unbatch_unquantize_model_dev", "decrypt_unquantize_model_dev", "decrypt_dev")

    def __init__(self, eng):
        self.eng, self.seen = eng, []
        for name in self.NAMES:
            setattr(eng, name, self._wrap(name, getattr(eng, name)))

    def _wrap(self, name, fn):
        def call(*a, **kw):
            self.seen.append(name)
            return fn(*a, **kw)
        return call

    def restore(self):
        for name in self.NAMES:
            delattr(self.eng, name)


def _round(clients, co, present, models, it, normalize, want_path, batch, n_ct, mask_pass):
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
    assert len(want_sum) == n_ct
    eng = co.cipher.engine
    _poison(eng, [16 * n_ct] * (len(present) + 2))
    np.random.set_state(state)
    up = co.quantize_encrypt([_W(dict(m)) for m in mine], normalize=normalize, present=present)
    assert up.path == want_path and up.present == present and len(up.ciphertexts) == len(present)
    assert _same_state(np.random.get_state(), want_state), "the NumPy stream must be left where the sequential steps leave it"
    for c in range(len(present)):
        assert up.ciphertexts[c].to_host().tobytes() == want[c].to_host().tobytes(), (it, present[c])
    assert up.partial_sum.to_host().tobytes() == want_sum.to_host().tobytes(), it
    assert co.shape_dict == here[0].shape_dict
    assert [float(a).hex() for a in co.quantizer.alpha_list] == [float(a).hex() for a in here[0].quantizer.alpha_list]
    assert (co.lead._cohort_mask is not None) == mask_pass
    # the decrypt: the first present client's own, told who uploaded
    here[0].set_idx_list(list(present))
    ref = here[0].decrypt_unquantize(_W({sorted(models[0])[0]: want_sum}), unnormalize=True)
    calls = _Calls(eng)
    try:
        got = co.decrypt_unquantize(unnormalize=True)
    finally:
        calls.restore()
    if mask_pass:
        assert calls.seen == ["combine_unbatch_unquantize_model_dev" if batch else "combine_unquantize_model_dev"], calls.seen
    else:
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


def _n_ct(sizes, bs):
    return sum(-(-s // bs) for s in sizes)


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_a_round_with_dropouts_is_the_present_clients_one_after_the_other(setting, pattern):
    b, batch = SETTINGS[setting]
    present = PATTERNS[pattern]
    sizes = _sizes(b, batch)
    clients, co = _make(b, batch)
    for it in range(2):
        models = _host_models(N_LOCAL, sizes, 100 + it)
        _round(clients, co, present, models, it, it == 1, "cohort-chain", batch, _n_ct(sizes, _bs(b, batch)), mask_pass=True)
    m = co.lead._cohort_mask
    runs = [(a, z + 1) for a, z in zip([p for p in present if p - 1 not in present], [p for p in present if p + 1 not in present])]
    assert (m[3], m[4]) == ([z for _a, z in runs], [a for a, _z in runs])


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_a_tiny_model_with_a_gap_takes_the_staged_chain_and_gives_the_same_bytes(setting):
    b, batch = SETTINGS[setting]
    sizes = _sizes(b, batch, tiny=True)
    clients, co = _make(b, batch)
    models = _host_models(N_LOCAL, sizes, 300)
    assert co.plan([_W(dict(models[p])) for p in (0, 1, 3, 4)], present=[0, 1, 3, 4]).path == "staged-chain"
    _round(clients, co, [0, 1, 3, 4], models, 2, False, "staged-chain", batch, _n_ct(sizes, _bs(b, batch)), mask_pass=False)


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_the_a_b_switch_runs_a_gapped_wide_cohort_staged_with_the_same_bytes(setting):
    """prefer = "staged-chain" (what the in-process A/B alternates): the gapped indices through the staged form at the chain's length."""
    b, batch = SETTINGS[setting]
    sizes = _sizes(b, batch)
    clients, co = _make(b, batch)
    co.prefer = "staged-chain"
    models = _host_models(N_LOCAL, sizes, 400)
    _round(clients, co, [0, 2, 3], models, 1, False, "staged-chain", batch, _n_ct(sizes, _bs(b, batch)), mask_pass=False)


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_a_precompute_job_with_a_gap_takes_the_prepared_cohort(setting):
    """The cohort's mask chain covers all five clients; the online launch is handed the present clients' masks and the whole cache is
    consumed."""
    b, batch = SETTINGS[setting]
    sizes = _sizes(b, batch, tiny=True) + [30001]
    n_ct = _n_ct(sizes, _bs(b, batch))
    clients, co = _make(b, batch, precompute_params=n_ct)
    it, present = 6, [0, 1, 3, 4]
    for cl in clients:
        cl.set_iter_index(it - 1)
    co.set_iter_index(it - 1)
    for cl in clients:
        cl.prepare_encrypt()
    co.prepare_encrypt()
    models = _host_models(N_LOCAL, sizes, 500)
    assert len(co._masks) == N_LOCAL
    for cl in clients:
        cl.set_iter_index(it)
    co.set_iter_index(it)
    # (_round sets the iteration again: the caches survive set_iter_index)
    assert co.plan([_W(dict(models[p])) for p in present], present=present).path == "prepared-cohort"
    _round(clients, co, present, models, it, False, "prepared-cohort", batch, n_ct, mask_pass=False)
    assert co._masks is None


def test_bad_present_lists_are_refused_and_leave_the_cohort_as_it_was():
    clients, co = _make(128, False)
    sizes = _sizes(128, False, tiny=True)
    models = _host_models(N_LOCAL, sizes, 600)
    up = _round(clients, co, [0, 1, 3, 4], models, 0, False, "staged-chain", False, sum(sizes), mask_pass=False)
    for present, count in (([1, 0], 2), ([0, 0], 2), ([0, 5], 2), ([0, 1], 3)):
        with pytest.raises(ValueError):
            co.quantize_encrypt([_W(dict(models[0])) for _ in range(count)], present=present)
    assert co._last is up
