"""GPU, class level: a precompute job's FlasheCohort -- prepare_encrypt() as one mask chain, quantize_encrypt as one online launch
("prepared-cohort") -- against n_local sequential precompute FlasheClients that each prepare their own masks: every ciphertext, the
partial sum, decrypt_unquantize's floats with and without prepare_decrypt(), shape_dict, alpha_list, the mean / std history and NumPy's
stream position, compared as bytes; the cache's life; the staged fallback; framework tensors."""
import numpy as np
import pytest

from test_gpu_cohort import KEY, _W, _host_models, _same_state

pytestmark = pytest.mark.gpu

IT = 6
SIZES = [1, 6, 0, 10007, 256 * 37 + 91, 10423]                         # 30001 values; no layer but the first starts on a multiple of 4

try:
    # (asked at collection: once a test has created an engine, the framework of the same process no longer finds its device)
    import torch as _torch_mod
    _TORCH_GPU = _torch_mod.cuda.is_available()
except ImportError:
    _TORCH_GPU = False


def _args(b, batch, n_ct):
    return {"quantize": {"int_bits": b, "batch": batch, "element_bits": 16, "padding": True, "secure": True},
            "precompute": {"enable": True, "num_params": n_ct}}


def _n_ct(sizes, b, batch, C):
    if not batch:
        return sum(sizes)
    bs = b // (16 + int(np.ceil(np.log2(C))))
    return sum((s + bs - 1) // bs for s in sizes)


def _vals(dv):
    """a ciphertext vector, one-limb, two-limb or compact, as flat uint64 words"""
    return np.asarray(dv.to_host()).astype(np.uint64).reshape(-1)


def _make(b, batch, compact, C, sizes=SIZES, num_params=None):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheClient, FlasheCohort
    cm.N_JOBS = 16
    args = _args(b, batch, _n_ct(sizes, b, batch, C) if num_params is None else num_params)
    clients = []
    for c in range(C):
        cl = FlasheClient(args)
        cl.create_cipher(c, C, KEY)
        clients.append(cl)
    co = FlasheCohort(args, first_idx=0, n_local=C, num_clients=C, prp_seed=KEY, compact=compact)
    return clients, co


def _sequential(clients, models, normalize, state, seeds):
    np.random.set_state(state)
    cts = []
    for c, (cl, m) in enumerate(zip(clients, models)):
        if seeds is not None:
            np.random.seed(seeds[c])
        w = cl.quantize_encrypt(_W(dict(m)), device=True, normalize=normalize)
        cts.append(w._weights[w.walking_order[0]])
    return cts, np.random.get_state()


def _encrypt_round(clients, co, models, it, normalize, seeds, want_path, cohort_models=None):
    """One upload of both sides from the same stream position; returns (the sequential clients' aggregate, the cohort's upload)."""
    np.random.seed(7 + it)
    np.random.random(3)                                               # an odd position in the stream
    state = np.random.get_state()
    want, want_state = _sequential(clients, models, normalize, state, seeds)
    want_sum = clients[0].cipher.aggregate(want)
    np.random.set_state(state)
    up = co.quantize_encrypt([_W(dict(m)) for m in (cohort_models or models)], normalize=normalize, seeds=seeds)
    assert up.path == want_path
    assert _same_state(np.random.get_state(), want_state), "the NumPy stream must be left where the sequential steps leave it"
    assert len(up.ciphertexts) == len(clients)
    for c in range(len(clients)):
        assert up.ciphertexts[c].compact == co.compact
        assert _vals(up.ciphertexts[c]).tobytes() == _vals(want[c]).tobytes(), (it, c)
    assert up.partial_sum.compact == co.compact
    assert _vals(up.partial_sum).tobytes() == _vals(want_sum).tobytes(), it
    assert co.shape_dict == clients[0].shape_dict
    assert [float(a).hex() for a in co.quantizer.alpha_list] == [float(a).hex() for a in clients[0].quantizer.alpha_list]
    return want_sum, up


def _decrypt_round(clients, co, models, want_sum, it, prepared):
    C = len(clients)
    if prepared:
        clients[0].prepare_decrypt()
        co.prepare_decrypt()
    clients[0].set_idx_list(list(range(C)))
    ref = clients[0].decrypt_unquantize(_W({sorted(models[0])[0]: want_sum}), unnormalize=True)
    got = co.decrypt_unquantize(unnormalize=True)
    assert got.walking_order == ref.walking_order
    for k in ref.walking_order:
        assert np.asarray(got._weights[k]).shape == np.asarray(ref._weights[k]).shape
        assert np.asarray(got._weights[k], dtype=np.float64).tobytes() == np.asarray(ref._weights[k], dtype=np.float64).tobytes(), (it, k)
    if prepared:
        assert co.cipher.next_iter_decrypt_prepared == {} and clients[0].cipher.next_iter_decrypt_prepared == {}
    qa, qb = co.quantizer, clients[0].quantizer
    assert [float(x).hex() for x in qa.past_layer_mean_list] == [float(x).hex() for x in qb.past_layer_mean_list]
    assert [float(x).hex() for x in qa.past_layer_std_list] == [float(x).hex() for x in qb.past_layer_std_list]
    for cl in clients[1:]:                                            # every client of the federation decrypts the same model: one state
        cl.quantizer.past_layer_mean_list = list(qb.past_layer_mean_list)
        cl.quantizer.past_layer_std_list = list(qb.past_layer_std_list)


def _set_iter(clients, co, it):
    for cl in clients:
        cl.set_iter_index(it)
    co.set_iter_index(it)


def _prepare(clients, co, it):
    """the job's order: the masks of iteration `it` are made at it - 1"""
    _set_iter(clients, co, it - 1)
    for cl in clients:
        cl.prepare_encrypt()
    co.prepare_encrypt()
    _set_iter(clients, co, it)


SETTINGS = [(128, False, False), (120, True, False), (20, False, False), (20, False, True)]


@pytest.mark.parametrize("seeded", [False, True], ids=["global-stream", "seeds"])
@pytest.mark.parametrize("C", [3, 10])
@pytest.mark.parametrize("b,batch,compact", SETTINGS)
def test_the_prepared_cohort_is_the_sequential_precompute_clients(b, batch, compact, C, seeded):
    """A first round on the masks create_cipher left (no cohort prepare_encrypt: "per-client"), then two consecutive rounds prepared one
    iteration ahead: one online launch each.  The seeded runs also normalise (the stage pass in front of the launch); the second prepared
    round decrypts with prepare_decrypt()."""
    clients, co = _make(b, batch, compact, C)
    normalize = seeded
    _set_iter(clients, co, IT - 2)
    for cl in clients + co._clients:                                  # the first round's masks: every client its own, as before
        cl.prepare_encrypt()
    _set_iter(clients, co, IT - 1)
    for rnd, it in enumerate((IT - 1, IT, IT + 1)):
        models = _host_models(C, SIZES, 100 + it)
        seeds = [1000 * it + c for c in range(C)] if seeded else None
        if rnd:
            _prepare(clients, co, it)
            assert co.plan([_W(dict(m)) for m in models]).path == "prepared-cohort"
            held = [cl.cipher.engine.prepared_query(cl.cipher.engine.PREPARED_ENCRYPT)[0] for cl in co._clients]
            assert not any(held), "the cohort's masks replace the clients' own add and minus vectors"
        want_sum, up = _encrypt_round(clients, co, models, it, normalize, seeds, "prepared-cohort" if rnd else "per-client")
        assert co._masks is None and co.plan([_W(dict(m)) for m in models]).path == "per-client"
        _decrypt_round(clients, co, models, want_sum, it, prepared=rnd == 2)


@pytest.mark.parametrize("b,batch,compact", [(128, False, False), (120, True, False), (20, False, True)])
def test_the_cache_is_consumed_once_and_the_next_step_is_the_clients_own(b, batch, compact):
    """After the prepared round a round without any prepare runs the clients' own online step ("per-client", AES) -- the same bytes as the
    sequential clients, which have no cache either -- and a round whose clients prepared on their own runs their prepared steps."""
    C = 3
    clients, co = _make(b, batch, compact, C)
    _prepare(clients, co, IT)
    models = _host_models(C, SIZES, 1)
    _encrypt_round(clients, co, models, IT, False, None, "prepared-cohort")
    assert co._masks is None
    _set_iter(clients, co, IT + 1)
    _encrypt_round(clients, co, _host_models(C, SIZES, 2), IT + 1, False, None, "per-client")
    for cl in clients + co._clients:                                  # the per-client precompute path, unchanged
        cl.prepare_encrypt()
    _set_iter(clients, co, IT + 2)
    _encrypt_round(clients, co, _host_models(C, SIZES, 3), IT + 2, False, None, "per-client")
    assert not any(cl.cipher.next_iter_encrypt_prepared for cl in co._clients)
    # a cache made for another iteration is consumed all the same (the reference does not check the iteration either)
    _set_iter(clients, co, IT + 3)
    for cl in clients:
        cl.prepare_encrypt()
    co.prepare_encrypt()
    _set_iter(clients, co, IT + 7)
    _encrypt_round(clients, co, _host_models(C, SIZES, 4), IT + 7, False, None, "prepared-cohort")


@pytest.mark.parametrize("b,batch,compact", [(128, False, False), (120, True, False), (20, False, True)])
@pytest.mark.parametrize("seeded", [False, True])
def test_a_cache_of_another_length_raises_the_sequential_steps_error_and_stays(b, batch, compact, seeded):
    C = 3
    n_ct = _n_ct(SIZES, b, batch, C)
    clients, co = _make(b, batch, compact, C, num_params=n_ct + 1)
    _prepare(clients, co, IT)
    models = _host_models(C, SIZES, 5)
    seeds = [31, 32, 33] if seeded else None
    np.random.seed(9)
    state = np.random.get_state()
    with pytest.raises(ValueError) as want:
        _sequential(clients, models, False, state, seeds)
    want_state = np.random.get_state()
    np.random.set_state(state)
    with pytest.raises(ValueError) as got:
        co.quantize_encrypt([_W(dict(m)) for m in models], seeds=seeds)
    assert str(got.value) == str(want.value) and "could not be broadcast" in str(got.value)
    assert _same_state(np.random.get_state(), want_state), "the stream stands where the first sequential client leaves it"
    assert co._masks is not None and len(co._masks[0]) == n_ct + 1 and co.plan([_W(dict(m)) for m in models]).path == "prepared-cohort"
    assert set(clients[0].cipher.next_iter_encrypt_prepared) == {"add", "minus"}


@pytest.mark.parametrize("b,batch,compact", SETTINGS)
def test_a_layer_that_is_float64_for_one_client_takes_the_staged_form(b, batch, compact):
    C = 3
    clients, co = _make(b, batch, compact, C)
    _prepare(clients, co, IT)
    models = _host_models(C, SIZES, 6)
    key = sorted(models[1])[3]                                        # the 10007-value layer: float64 for client 1 only
    assert models[0][key].dtype == np.float64 and models[0][key].size == 10007
    models[1][key] = models[1][key].astype(np.float32)
    plan = co.plan([_W(dict(m)) for m in models])
    assert plan.path == "prepared-staged" and "float64 for some clients only" in plan.reason
    _encrypt_round(clients, co, models, IT, False, None, "prepared-staged")
    assert co._masks is None
    # the A/B switch takes the same form on a model that would run the one launch: the same bytes
    _prepare(clients, co, IT + 1)
    co.prefer = "staged-chain"
    _encrypt_round(clients, co, _host_models(C, SIZES, 7), IT + 1, True, None, "prepared-staged")


@pytest.mark.parametrize("b,batch,compact", SETTINGS)
def test_framework_tensors_mixed_with_host_layers(b, batch, compact):
    """float32 and bfloat16 layers as framework device tensors (the cohort reads them where they lie; bfloat16 through the stage pass),
    the others host arrays: the bytes of the sequential clients fed the same tensors."""
    torch = pytest.importorskip("torch")
    if not (_TORCH_GPU and torch.cuda.is_available()):
        pytest.skip("no GPU visible to torch")
    C = 3
    clients, co = _make(b, batch, compact, C)
    _prepare(clients, co, IT)
    models = _host_models(C, SIZES, 8, dtypes=("float32",))
    names = sorted(models[0])
    for m in models:
        m[names[3]] = torch.from_numpy(m[names[3]]).to("cuda")
        m[names[4]] = torch.from_numpy(m[names[4]]).to("cuda").to(torch.bfloat16)
        m[names[5]] = m[names[5]].astype(np.float64)
    torch.cuda.synchronize()
    _encrypt_round(clients, co, models, IT, True, None, "prepared-cohort")
