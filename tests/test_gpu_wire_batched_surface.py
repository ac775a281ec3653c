"""GPU: packed="fused" through the Python surface.  A batched job at int_bits 120 / 128 uploads in one launch (path "fused") the integer
packed=True and compress() give; a three-client wire round returns the unpacked round's floats as bytes; int_bits 40 reports "fused" too."""
import numpy as np
import pytest

from test_gpu_wire_python_surface import C, SHAPES, _W, _client, _upload

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("b", [120, 128])
def test_fused_batched_upload_is_the_staged_one(b):
    from flashe_amd.engine import PackedVector
    from flashe_amd.weights import TransferableWeights
    cl = _client(b, 1, True)
    pv, staged, ct = _upload(cl, 3, packed="fused"), _upload(cl, 3, packed=True), _upload(cl, 3)
    assert isinstance(pv, PackedVector) and pv.path == "fused" and staged.path == "staged" and len(pv) == len(ct)
    assert pv.to_int() == staged.to_int() == TransferableWeights({"w": ct}, b).unboxed["w"] == _upload(cl, 3, packed="fused", device=False)


def test_fused_batched_upload_from_framework_tensors_is_the_host_one():
    from test_gpu_wire_python_surface import _model
    cl = _client(120, 1, True)

    class Dev:                                   # a device array by __cuda_array_interface__, held in the engine's own memory
        def __init__(self, v):
            self.buf = cl.cipher.engine.upload(v.reshape(-1))
            self.__cuda_array_interface__ = {"shape": v.shape, "typestr": v.dtype.str, "data": (self.buf.ptr, False), "version": 3}
    np.random.seed(3)
    w = cl.quantize_encrypt(_W({k: Dev(v) for k, v in _model(3).items()}), packed="fused")
    pv = w._weights[w.walking_order[0]]
    assert pv.path == "fused" and pv.to_int() == _upload(cl, 3, packed="fused").to_int()


@pytest.mark.parametrize("b,present,min_elems", [(120, (0, 1, 2), 0), (128, (0, 1, 2), 0), (120, (0, 2), 0), (120, (0, 1, 2), None)])
def test_a_batched_round_in_the_wire_form_returns_the_unpacked_rounds_floats(monkeypatch, b, present, min_elems):
    """min_elems 0: decrypt_unquantize takes its one launch at this small model too; the library declines the two add prefixes a
    dropped-out client leaves, and the staged launches run.  None: the measured threshold, under which the model stays staged."""
    from flashe_amd import block
    from flashe_amd.engine import PackedVector
    if min_elems is not None:
        monkeypatch.setattr(block, "_WIDE_WIRE_BACK_MIN_ELEMS", min_elems)
    clients = [_client(b, i, True) for i in range(C)]
    plain = [_upload(clients[i], 10 + i) for i in present]
    wire = [_upload(clients[i], 10 + i, packed="fused") for i in present]
    assert all(p.path == "fused" for p in wire)
    lead = clients[0]
    agg, agg_w = lead.cipher.aggregate(plain, packed=True), lead.cipher.aggregate(wire, packed=True)
    assert isinstance(agg_w, PackedVector)
    eng, took = lead.cipher.engine, []
    fused = eng.unpack_decrypt_unbatch_unquantize_model_dev
    monkeypatch.setattr(eng, "unpack_decrypt_unbatch_unquantize_model_dev", lambda *a: took.append(fused(*a)) or took[-1])
    lead.set_idx_list(list(present))
    want = lead.decrypt_unquantize(_W({"a": agg}))
    lead.set_idx_list(list(present))
    got = lead.decrypt_unquantize(_W({"a": agg_w}))
    assert took == ([] if min_elems is None else [len(present) == C])
    for k in SHAPES:
        assert got._weights[k].tobytes() == want._weights[k].tobytes(), k


def test_an_unbatched_client_above_32_bits_takes_its_one_launch_when_asked():
    cl = _client(40, 1)
    pv = _upload(cl, 3, packed="fused")
    assert pv.path == "fused" and _upload(cl, 3, packed=True).path == "staged" and pv.to_int() == _upload(cl, 3, packed=True).to_int()
