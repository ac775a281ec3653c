"""GPU: a three-client wire round in which client 1 dropped out (set_idx_list leaves two add and two minus prefixes) through
FlasheClient.decrypt_unquantize: the packed sum reaches the floats of the unpacked round, as bytes, through the lists launch where the
routing constants admit it, and through the staged launches under the constants as shipped when they do not."""
import pytest

from test_gpu_wire_python_surface import C, SHAPES, _W, _client, _upload

pytestmark = pytest.mark.gpu
PRESENT = (0, 2)


@pytest.mark.parametrize("admit", [True, False])
@pytest.mark.parametrize("b,batch", [(20, False), (120, True)])
def test_a_round_with_a_dropout_returns_the_unpacked_rounds_floats(monkeypatch, b, batch, admit):
    from flashe_amd import block
    if admit:
        for name in ("_WIRE_LISTS_MIN_ELEMS", "_WIDE_WIRE_LISTS_MIN_ELEMS"):
            monkeypatch.setattr(block, name, 0)
        for name in ("_WIRE_LISTS_MAX_PREFIXES", "_WIDE_WIRE_LISTS_MAX_PREFIXES"):
            monkeypatch.setattr(block, name, 192)
    clients = [_client(b, i, batch) for i in range(C)]
    plain = [_upload(clients[i], 10 + i) for i in PRESENT]
    wire = [_upload(clients[i], 10 + i, packed="fused") for i in PRESENT]
    lead = clients[0]
    agg, agg_w = lead.cipher.aggregate(plain, packed=True), lead.cipher.aggregate(wire, packed=True)
    eng, took = lead.cipher.engine, []
    name = "unpack_decrypt_lists_unbatch_unquantize_model_dev" if batch else "unpack_decrypt_lists_unquantize_model_dev"
    fused = getattr(eng, name)
    monkeypatch.setattr(eng, name, lambda *a: took.append(fused(*a)) or took[-1])
    lead.set_idx_list(list(PRESENT))
    want = lead.decrypt_unquantize(_W({"a": agg}))
    lead.set_idx_list(list(PRESENT))
    got = lead.decrypt_unquantize(_W({"a": agg_w}))
    assert took == ([True] if admit else [])              # (the model is far below the shipped smallest size)
    for k in SHAPES:
        assert got._weights[k].tobytes() == want._weights[k].tobytes(), k
