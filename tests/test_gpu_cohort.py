"""GPU: a cohort of co-located clients (flashe_amd.block.FlasheCohort) against the reference's recorded client steps and against the
same clients run one after the other as FlasheClients in one process -- every ciphertext, their sum, NumPy's generator, the decrypted
floats and the quantiser's history, compared as bytes.  `up.path` is asserted everywhere so that a silent mis-route shows."""
import numpy as np
import pytest

from conftest import load_golden, unhex

pytestmark = pytest.mark.gpu

KEY = bytes(range(32))


class _W:
    def __init__(self, layers):
        self.walking_order = sorted(layers)
        self._weights = dict(layers)


def _arr(hexstr, dtype, shape):
    return np.frombuffer(bytes.fromhex(hexstr), dtype=dtype).copy().reshape(shape)


def _args(b, eb=16, batch=False):
    return {"quantize": {"int_bits": b, "batch": batch, "element_bits": eb, "padding": True, "secure": True}, "precompute": {"enable": False}}


def _poison(eng, sizes):
    """Blocks of the sizes the next call allocates, filled with a pattern and handed back to the engine's pool."""
    bufs = [eng.alloc(s) for s in sizes]
    for b, s in zip(bufs, sizes):
        eng.memset_dev(b, 0xA5, s)
    eng.sync()
    for b in bufs:
        b.free()


# ------------------------------------------------------------------------------------------------ the reference's recorded steps
@pytest.mark.parametrize("case_i", range(8))
def test_cohort_is_the_reference_jobs_client_steps(case_i):
    """The eight dense cases of tests/golden/clientstep.json (recorded by calling the reference: per-client seeds, b = 128 / 64 / 20 / 23 /
    120, single and double mask, batched and not) through one FlasheCohort: every flat ciphertext, the element-wise aggregate as
    partial_sum, alpha_list, shape_dict and the floats of decrypt_unquantize equal the fixture byte for byte.  The vectors are tiny, so
    every case takes the staged fallback."""
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheCohort
    from oracle.flashe_oracle import limbs_to_ints
    case = load_golden("clientstep.json")["dense"][case_i]
    b, C = case["b"], case["num_clients"]
    cm.N_JOBS = case["n_jobs"]
    co = FlasheCohort(_args(b, case["element_bits"], bool(case.get("batch"))), first_idx=0, n_local=C, num_clients=C, prp_seed=KEY)
    co.cipher.masking_scheme = case["scheme"]
    co.set_iter_index(case["iter"])
    ws = [_W({nm: _arr(rec["layers"][nm], np.dtype(dt), sh) for nm, sh, dt in case["layers"]}) for rec in case["clients"]]
    up = co.quantize_encrypt(ws, seeds=[rec["seed"] for rec in case["clients"]])
    assert up.path == "staged-chain"
    assert len(up.ciphertexts) == C
    for c, rec in enumerate(case["clients"]):
        assert limbs_to_ints(up.ciphertexts[c].to_host()) == unhex(rec["flat_ct"]), (b, c)
        assert [float(a).hex() for a in co.quantizer.alpha_list] == rec["alpha"]
        assert {k: list(sh) for k, sh in co.shape_dict.items()} == rec["shape_dict"]
    assert limbs_to_ints(up.partial_sum.to_host()) == unhex(case["agg_elem"])
    back = co.decrypt_unquantize()
    assert back.walking_order == sorted(nm for nm, _sh, _dt in case["layers"])
    for nm, sh, _dt in case["layers"]:
        a = back._weights[nm]
        assert a.shape == tuple(sh)
        assert np.asarray(a, dtype=np.float64).tobytes() == bytes.fromhex(case["out_elem"]["unquantized"][nm]), (b, nm)


# ------------------------------------------------------------------------------------------------ against sequential FlasheClients
def _cu_count():
    from flashe_amd import Engine
    return Engine(KEY, 128).cu_count


def _model_sizes(n):
    """Many layers of n values in all: one value, an odd prime, a size that ends mid-tile, an empty layer, then the rest in uneven cuts."""
    head = [1, 10007, 256 * 37 + 91, 0]
    rest = n - sum(head)
    cuts = [rest // 7, rest // 3 + 5, rest // 5 - 3]
    return head + cuts + [rest - sum(cuts)]


def _host_models(C, sizes, seed, dtypes=("float32", "float64")):
    g = np.random.Generator(np.random.PCG64(seed))
    return [{f"l{i:02d}": (g.standard_normal(s) * 0.05 + 0.01 * c).astype(dtypes[i % len(dtypes)]).reshape((s,) if i % 2 else (1, s))
             for i, s in enumerate(sizes)} for c in range(C)]


def _sequential(clients, models, normalize, state):
    """One round of the clients' own steps in one process, NumPy's generator starting from `state`."""
    np.random.set_state(state)
    cts = []
    for cl, m in zip(clients, models):
        w = cl.quantize_encrypt(_W(dict(m)), device=True, normalize=normalize)
        cts.append(w._weights[w.walking_order[0]])
    return cts, np.random.get_state()


def _same_state(a, b):
    return a[0] == b[0] and a[2] == b[2] and np.array_equal(a[1], b[1])


def _round_trip(C, n, normalize, rounds, first_idx=0, num_clients=None, want_path="cohort-chain"):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheClient, FlasheCohort
    cm.N_JOBS = 16
    num_clients = C if num_clients is None else num_clients
    sizes = _model_sizes(n)
    clients = []
    for c in range(C):
        cl = FlasheClient(_args(128))
        cl.create_cipher(first_idx + c, num_clients, KEY)
        clients.append(cl)
    co = FlasheCohort(_args(128), first_idx=first_idx, n_local=C, num_clients=num_clients, prp_seed=KEY)
    eng = co.cipher.engine
    for it in range(rounds):
        models = _host_models(C, sizes, 100 + it)
        for cl in clients:
            cl.set_iter_index(it)
        co.set_iter_index(it)
        np.random.seed(7 + it)
        np.random.random(3)                                   # an odd position in the stream
        state = np.random.get_state()
        want, want_state = _sequential(clients, models, normalize, state)
        want_sum = clients[0].cipher.aggregate(want)
        _poison(eng, [16 * n] * (C + 2))
        np.random.set_state(state)
        up = co.quantize_encrypt([_W(dict(m)) for m in models], normalize=normalize)
        assert up.path == want_path
        assert _same_state(np.random.get_state(), want_state), "the NumPy stream must be left where the sequential steps leave it"
        for c in range(C):
            assert up.ciphertexts[c].to_host().tobytes() == want[c].to_host().tobytes(), (it, c)
        assert up.partial_sum.to_host().tobytes() == want_sum.to_host().tobytes(), it
        assert co.shape_dict == clients[0].shape_dict
        assert [float(a).hex() for a in co.quantizer.alpha_list] == [float(a).hex() for a in clients[0].quantizer.alpha_list]
        if num_clients != C:
            with pytest.raises(ValueError):
                co.decrypt_unquantize()
            return
        clients[0].set_idx_list(list(range(C)))
        ref = clients[0].decrypt_unquantize(_W({sorted(models[0])[0]: want_sum}), unnormalize=True)
        got = co.decrypt_unquantize(unnormalize=True)
        assert got.walking_order == ref.walking_order
        for k in ref.walking_order:
            assert np.asarray(got._weights[k]).shape == np.asarray(ref._weights[k]).shape
            assert np.asarray(got._weights[k], dtype=np.float64).tobytes() == np.asarray(ref._weights[k], dtype=np.float64).tobytes(), (it, k)
        qa, qb = co.quantizer, clients[0].quantizer
        assert [float(x).hex() for x in qa.past_layer_mean_list] == [float(x).hex() for x in qb.past_layer_mean_list]
        assert [float(x).hex() for x in qa.past_layer_std_list] == [float(x).hex() for x in qb.past_layer_std_list]
        for cl in clients[1:]:                                # every client of the federation decrypts the same model: one state
            cl.quantizer.past_layer_mean_list = list(qb.past_layer_mean_list)
            cl.quantizer.past_layer_std_list = list(qb.past_layer_std_list)


@pytest.mark.parametrize("C", [1, 2, 10])
@pytest.mark.parametrize("normalize", [False, True])
def test_chained_cohort_is_the_sequential_clients_for_three_rounds(C, normalize):
    """The fused launch (model just past the summed chain's admission length for this chip) against C FlasheClients, three rounds."""
    from flashe_amd.block import cohort_admission_length
    _round_trip(C, cohort_admission_length(_cu_count()) + 12345, normalize, rounds=3)


def test_one_element_below_the_admission_length_takes_the_staged_chain():
    from flashe_amd.block import cohort_admission_length
    n = cohort_admission_length(_cu_count())
    _round_trip(3, n, True, rounds=1)
    _round_trip(3, n - 1, True, rounds=1, want_path="staged-chain")


def test_a_cohort_inside_a_larger_federation_writes_a_partial_aggregate():
    from flashe_amd.block import cohort_admission_length
    _round_trip(4, cohort_admission_length(_cu_count()) + 77, False, rounds=1, first_idx=3, num_clients=9)


@pytest.mark.parametrize("C, path", [(128, "cohort-chain"), (129, "staged-chain")])
def test_the_link_table_boundary(C, path):
    """kMaxLinks outputs chain; one more takes the fallback.  The sequential side is one FlasheClient whose cipher takes each client's
    index in turn."""
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheClient, FlasheCohort, cohort_admission_length
    cm.N_JOBS = 16
    n = cohort_admission_length(_cu_count()) + 300
    sizes = [n - 999, 0, 999]
    g = np.random.Generator(np.random.PCG64(C))
    base = [(g.standard_normal(s) * 0.05).astype(np.float32) for s in sizes]
    models = [{f"l{i}": b + np.float32(0.001 * c) for i, b in enumerate(base)} for c in range(C)]
    cl = FlasheClient(_args(128))
    cl.create_cipher(0, C, KEY)
    cl.set_iter_index(2)
    np.random.seed(C)
    state = np.random.get_state()
    want = []
    for c in range(C):
        cl.cipher.idx = c
        w = cl.quantize_encrypt(_W(dict(models[c])), device=True)
        want.append(w._weights[w.walking_order[0]])
    want_state = np.random.get_state()
    cl.cipher.idx = 0
    want_sum = cl.cipher.aggregate(want)
    co = FlasheCohort(_args(128), first_idx=0, n_local=C, num_clients=C, prp_seed=KEY)
    co.set_iter_index(2)
    np.random.set_state(state)
    up = co.quantize_encrypt([_W(dict(m)) for m in models])
    assert up.path == path
    assert _same_state(np.random.get_state(), want_state)
    for c in range(C):
        assert up.ciphertexts[c].to_host().tobytes() == want[c].to_host().tobytes(), c
    assert up.partial_sum.to_host().tobytes() == want_sum.to_host().tobytes()
    cl.set_idx_list(list(range(C)))
    ref = cl.decrypt_unquantize(_W({"l0": want_sum}))
    got = co.decrypt_unquantize()
    for k in ref.walking_order:
        assert np.asarray(got._weights[k], dtype=np.float64).tobytes() == np.asarray(ref._weights[k], dtype=np.float64).tobytes(), k


def test_the_a_b_switch_and_mismatched_clients():
    """FLASHE_CHAIN=0 is read when the engine is created: the planner routes such a cohort to the staged form.  Mismatched Weights and
    sparse uploads are refused before any work."""
    import os
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheCohort, cohort_admission_length
    cm.N_JOBS = 16
    n = cohort_admission_length(_cu_count()) + 5
    co = FlasheCohort(_args(128), first_idx=0, n_local=2, num_clients=2, prp_seed=KEY)
    co.set_iter_index(0)
    a = {"w": np.zeros(n, np.float32)}
    with pytest.raises(ValueError, match="client 1"):
        co.quantize_encrypt([_W(dict(a)), _W({"w": np.zeros(n - 1, np.float32)})])
    with pytest.raises(TypeError):
        co.quantize_encrypt([_W(dict(a)), _W({"w": np.zeros(n, np.float32), "zzz": np.zeros(1)})])
    with pytest.raises(ValueError):
        co.quantize_encrypt([_W(dict(a))])
    old = os.environ.get("FLASHE_CHAIN")
    os.environ["FLASHE_CHAIN"] = "0"
    try:
        assert co.plan([_W(dict(a)), _W(dict(a))]).path == "staged-chain"
    finally:
        if old is None:
            del os.environ["FLASHE_CHAIN"]
        else:
            os.environ["FLASHE_CHAIN"] = old
    assert co.plan([_W(dict(a)), _W(dict(a))]).path == "cohort-chain"
