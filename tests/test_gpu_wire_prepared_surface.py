"""GPU: a FlasheClient precompute round through the wire form.  quantize_encrypt(packed="fused") with a consumed encrypt cache uploads in ONE
launch (path "fused"), aggregate(packed=True) sums the integers, and decrypt_unquantize takes the packed sum back in one launch with the
prepared decrypt masks: the floats are, byte for byte, those of the same round with packed=True -- the staged route -- and both caches are
consumed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEY = bytes(range(32))
IT, C, EB = 6, 3, 16
SHAPES = {"a": (7,), "b": (300, 3), "c": (41,)}


class _W:
    def __init__(self, layers):
        self.walking_order = sorted(layers)
        self._weights = dict(layers)


def _client(b, idx, batch):
    """A precompute client at iteration IT whose encrypt masks were prepared in the job's order: at IT - 1, for IT."""
    from flashe_amd.block import FlasheClient
    bs = b // (EB + int(np.ceil(np.log2(C))))
    n_ct = sum((int(np.prod(s)) + bs - 1) // bs if batch else int(np.prod(s)) for s in SHAPES.values())
    cl = FlasheClient({"quantize": {"int_bits": b, "batch": batch, "element_bits": EB, "padding": True, "secure": True},
                       "precompute": {"enable": True, "num_params": n_ct}})
    cl.create_cipher(idx, C, KEY)
    cl.cipher.masking_scheme = "double"
    cl.set_iter_index(IT - 1)
    cl.prepare_encrypt()
    cl.set_iter_index(IT)
    return cl


def _round(b, batch, packed, took):
    """(the uploads, the lead client's floats) of one round of C clients with `packed`."""
    from flashe_amd import cipher as cm
    cm.N_JOBS = 16
    clients, ups = [_client(b, c, batch) for c in range(C)], []
    for c, cl in enumerate(clients):
        rs = np.random.RandomState(40 + c)
        model = {k: rs.normal(0.0, 0.05, s).astype(np.float64 if k == "a" else np.float32) for k, s in SHAPES.items()}
        np.random.seed(7 + c)
        w = cl.quantize_encrypt(_W(model), device=True, packed=packed)
        ups.append(w._weights[w.walking_order[0]])
        assert not cl.cipher.engine.prepared_query(cl.cipher.engine.PREPARED_ENCRYPT)[0], "the encrypt cache is consumed"
    lead = clients[0]
    eng = lead.cipher.engine
    agg = lead.cipher.aggregate(ups, packed=True)
    lead.prepare_decrypt()
    lead.set_idx_list(list(range(C)))
    for name in ("unpack_decrypt_prepared_unquantize_model_dev", "unpack_decrypt_prepared_unbatch_unquantize_model_dev"):
        fused = getattr(eng, name)
        setattr(eng, name, lambda *a, fused=fused: took.append(fused(*a)) or took[-1])
    back = lead.decrypt_unquantize(_W({"a": agg}))
    assert not eng.prepared_query(eng.PREPARED_DECRYPT)[0], "the decrypt cache is consumed"
    return ups, back


@pytest.mark.parametrize("b,batch", [(20, False), (120, True)])
def test_a_precompute_round_in_the_wire_form_is_the_staged_round(b, batch):
    took_f, took_s = [], []
    ups_f, got = _round(b, batch, "fused", took_f)
    ups_s, want = _round(b, batch, True, took_s)
    assert all(p.path == "fused" for p in ups_f) and all(p.path == "staged" for p in ups_s)
    assert [p.to_int() for p in ups_f] == [p.to_int() for p in ups_s]
    assert took_f == [True] and took_s == [], "the way back follows the upload's request"
    for k in SHAPES:
        assert got._weights[k].tobytes() == want._weights[k].tobytes(), k
