"""GPU: packed=True through the Python surface -- FlasheClient.quantize_encrypt / decrypt_unquantize, FlasheCipher.aggregate,
TransferableWeights -- against the same seeded calls without it: the packed integer equals compress() of the unpacked ciphertext, and a
three-client round in the wire form returns the unpacked round's floats as bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEY = bytes(range(32))
SHAPES = {"a": (7,), "b": (3, 43), "c": (1031,)}
C = 3


class _W:
    def __init__(self, layers):
        self.walking_order = sorted(layers)
        self._weights = dict(layers)


def _client(b, idx, batch=False):
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheClient
    cm.N_JOBS = 16
    cl = FlasheClient({"quantize": {"int_bits": b, "batch": batch, "element_bits": 16, "padding": True, "secure": True},
                       "precompute": {"enable": False, "num_params": None}})
    cl.create_cipher(idx, C, KEY)
    cl.set_iter_index(5)
    q = cl.quantizer
    q.layer_size_list = [int(np.prod(s)) for s in SHAPES.values()]
    q.past_layer_mean_list = [np.float64(0.0123 * (i + 1)) for i in range(len(SHAPES))]
    q.past_layer_std_list = [np.float64(0.05) for _ in SHAPES]
    return cl


def _model(seed):
    rs = np.random.RandomState(seed)
    return {k: rs.normal(0.0, 0.05, s).astype(np.float64 if k == "a" else np.float32) for k, s in SHAPES.items()}


def _upload(cl, seed, **kw):
    np.random.seed(seed)
    w = cl.quantize_encrypt(_W(_model(seed)), **kw)
    return w._weights[w.walking_order[0]]


@pytest.mark.parametrize("b,batch,path", [(20, False, "fused"), (128, True, "staged")])
def test_packed_upload_is_compress_of_the_unpacked_one(b, batch, path):
    from flashe_amd.engine import PackedVector
    from flashe_amd.weights import TransferableWeights, from_big_int, to_big_int
    cl = _client(b, 1, batch)
    pv = _upload(cl, 3, packed=True)
    ct = _upload(cl, 3)
    assert isinstance(pv, PackedVector) and pv.path == path and len(pv) == len(ct)
    want = TransferableWeights({"w": ct}, b).unboxed["w"]
    assert pv.to_int() == want == _upload(cl, 3, packed=True, device=False)
    # the wire form passes compress / decompress with no pack or unpack launch, and refuses another width
    tw = TransferableWeights({"w": pv}, b)
    assert tw.unboxed["w"] == want
    back = tw.decompress(as_device="packed")["w"]
    assert isinstance(back, PackedVector) and back.to_int() == want and (len(back), back.bits) == (len(ct), b)
    assert from_big_int(want, len(ct), b, as_device="packed").to_int() == want
    with pytest.raises(ValueError):
        to_big_int(pv, b + 1)


def test_a_round_in_the_wire_form_returns_the_unpacked_rounds_floats():
    from flashe_amd.engine import PackedVector
    clients = [_client(20, i) for i in range(C)]
    plain = [_upload(cl, 10 + i) for i, cl in enumerate(clients)]
    wire = [_upload(cl, 10 + i, packed=True) for i, cl in enumerate(clients)]
    assert all(p.path == "fused" for p in wire)
    lead = clients[0]
    agg, agg_w = lead.cipher.aggregate(plain, packed=True), lead.cipher.aggregate(wire, packed=True)
    assert isinstance(agg_w, PackedVector)
    with pytest.raises(TypeError):
        lead.cipher.aggregate([wire[0], plain[1]], packed=True)
    lead.set_idx_list(list(range(C)))
    want = lead.decrypt_unquantize(_W({"a": agg}))
    got = lead.decrypt_unquantize(_W({"a": agg_w}))
    for k in SHAPES:
        assert got._weights[k].tobytes() == want._weights[k].tobytes(), k
