"""CPU: which engine calls cipher.aggregate(..., packed=True) makes.  The engine is the oracle-backed double of tests/fake_engine.py
extended HERE with the two new methods (computed by tests/packed_elems_ref.py) and a record of every call: the new method is called once
when it exists, the pack / reduce / unpack sequence runs when it is missing or declines (FLASHE_ENOTSUP -> False), compact operands are
not widened (only the result is, into the one-limb layout packed=True has always returned; the cohort's _compact_result=True keeps it
uint32), and the results are the same values either way.  Also pins decrypt_unquantize(packed=True, aggregate=...) as a ValueError."""
import numpy as np
import pytest

import packed_elems_ref as R
from fake_engine import OracleEngine

from flashe_amd import cipher as cm
from flashe_amd.engine import DeviceVector


class RecordingEngine(OracleEngine):
    """OracleEngine + the compact layout's reduce and widen / narrow on FakeBufs; `calls` lists every method of interest in order."""
    WATCH = ("pack_dev", "unpack_dev", "aggregate_packed_dev", "widen_u32_dev", "narrow_u32_dev", "aggregate_elem_u32_dev")

    def __init__(self, key, int_bits, device=0, stream=None):
        super().__init__(key, int_bits, device, stream)
        self.calls = []

    def __getattribute__(self, name):
        val = object.__getattribute__(self, name)
        if name in type(self).WATCH or name.startswith("aggregate_packed_elems"):
            calls = object.__getattribute__(self, "calls")

            def call(*a, **kw):
                calls.append(name)
                return val(*a, **kw)
            return call
        return val

    def aggregate_elem_u32_dev(self, cts, n, out):
        out.arr = (sum(c.arr.reshape(-1)[:n].astype(np.uint64) for c in cts) & np.uint64((1 << self.int_bits) - 1)).astype(np.uint32)

    def widen_u32_dev(self, n, inp, out):
        out.arr = inp.arr.view(np.uint32).reshape(-1)[:n].astype(np.uint64).reshape(n, 1)

    def narrow_u32_dev(self, n, inp, out):
        out.arr = inp.arr.view(np.uint64).reshape(-1)[:n].astype(np.uint32)


class NewEngine(RecordingEngine):
    """... + the two new calls.  declines: what they answer with (False = FLASHE_ENOTSUP, nothing written)."""
    takes = True

    def aggregate_packed_elems_dev(self, cts, n, out):
        if not self.takes:
            return False
        ops = [[int(v) for v in R.limbs_to_ints(np.ascontiguousarray(c.arr).view(np.uint64).reshape(n, self.limbs))] for c in cts]
        out.arr = R.to_array(R.reference(self.int_bits, ops), 8 * self.limbs).reshape(n, self.limbs)
        return True

    def aggregate_packed_elems_u32_dev(self, cts, n, out):
        if not self.takes:
            return False
        ops = [[int(v) for v in c.arr.view(np.uint32).reshape(-1)[:n]] for c in cts]
        out.arr = R.to_array(R.reference(self.int_bits, ops), 4)
        return True


def _ints(res):
    a = res.to_host() if isinstance(res, DeviceVector) else np.asarray(res)
    if a.dtype == np.uint32:
        return [int(v) for v in a.reshape(-1)]
    a = a.reshape(len(a), -1)
    return [int(r[0]) | (int(r[1]) << 64 if a.shape[1] == 2 else 0) for r in a]


@pytest.mark.parametrize("b", [20, 64, 128])
def test_packed_aggregate_takes_the_new_call_once_and_falls_back_without_it(oracle, b):
    n, C = 77, 3
    ops = [[v & ((1 << b) - 1) for v in o] for o in R.random_ops(b, n, C)]
    arrs = [R.to_array(o, 16 if b > 64 else 8).reshape(n, -1) for o in ops]
    want = R.reference(b, ops)
    new, old, declining = NewEngine(R.KEY, b), RecordingEngine(R.KEY, b), NewEngine(R.KEY, b)
    declining.takes = False
    got = cm.aggregate(arrs, b, packed=True, _engine=new)
    assert _ints(got) == want and new.calls == ["aggregate_packed_elems_dev"]
    got = cm.aggregate([DeviceVector.from_host(new, a) for a in arrs], b, packed=True, _engine=new)
    assert isinstance(got, DeviceVector) and _ints(got) == want and new.calls == ["aggregate_packed_elems_dev"] * 2
    # an engine without the method (the oracle-backed double as it is): today's sequence, untouched
    got = cm.aggregate(arrs, b, packed=True, _engine=old)
    assert _ints(got) == want and old.calls == ["pack_dev"] * C + ["aggregate_packed_dev", "unpack_dev"]
    # the library declines: asked once, then the same sequence
    got = cm.aggregate(arrs, b, packed=True, _engine=declining)
    assert _ints(got) == want and declining.calls == ["aggregate_packed_elems_dev"] + ["pack_dev"] * C + ["aggregate_packed_dev", "unpack_dev"]
    # the element-wise reduce never asks
    new.calls.clear()
    cm.aggregate(arrs, b, packed=False, _engine=new)
    assert new.calls == []


@pytest.mark.parametrize("b", [16, 20, 32])
def test_compact_operands_are_not_widened(oracle, b):
    n, C = 300, 4
    ops = [[v & ((1 << b) - 1) for v in o] for o in R.random_ops(b, n, C, compact=True)]
    want = R.reference(b, ops)
    new, old, declining = NewEngine(R.KEY, b), RecordingEngine(R.KEY, b), NewEngine(R.KEY, b)
    declining.takes = False
    u32 = [R.to_array(o, 4) for o in ops]
    got = cm.aggregate(u32, b, packed=True, _engine=new)            # uint32 arrays in: reduced as they are, the RESULT widened as ever
    assert got.dtype == np.uint64 and got.shape == (n,) and _ints(got) == want and new.calls == ["aggregate_packed_elems_u32_dev", "widen_u32_dev"]
    assert got.tobytes() == cm.aggregate(u32, b, packed=True, _engine=old).tobytes()
    old.calls.clear()
    new.calls.clear()
    got = cm.aggregate([DeviceVector.from_host(new, a) for a in u32], b, packed=True, _engine=new)
    assert not got.compact and _ints(got) == want and new.calls == ["aggregate_packed_elems_u32_dev", "widen_u32_dev"]
    new.calls.clear()
    got = cm.aggregate([DeviceVector.from_host(new, a) for a in u32], b, packed=True, _engine=new, _compact_result=True)     # the cohort's form
    assert got.compact and _ints(got) == want and new.calls == ["aggregate_packed_elems_u32_dev"]
    got = cm.aggregate(u32, b, packed=True, _engine=new, _compact_result=True)
    assert got.dtype == np.uint32 and _ints(got) == want
    # one one-limb operand among them: the one-limb call on widened operands
    new.calls.clear()
    got = cm.aggregate([u32[0].astype(np.uint64)] + [DeviceVector.from_host(new, a) for a in u32[1:]], b, packed=True, _engine=new, keep_on_device=True)
    assert not got.compact and _ints(got) == want and new.calls == ["widen_u32_dev"] * (C - 1) + ["aggregate_packed_elems_dev"]
    # without the method, and when it declines: widened, packed, reduced, unpacked -- the same values
    for eng, head in ((old, []), (declining, ["aggregate_packed_elems_u32_dev"])):
        got = cm.aggregate([DeviceVector.from_host(eng, a) for a in u32], b, packed=True, _engine=eng)
        assert _ints(got) == want
        tail = ["aggregate_packed_elems_dev"] if eng is declining else []
        assert eng.calls == head + ["widen_u32_dev"] * C + tail + ["pack_dev"] * C + ["aggregate_packed_dev", "unpack_dev"], eng.calls


def test_packed_decrypt_of_a_given_aggregate_is_refused(oracle, monkeypatch):
    from flashe_amd.block import FlasheCohort
    monkeypatch.setattr(cm.FlasheCipher, "_engine_cls", NewEngine)
    args = {"quantize": {"int_bits": 128, "batch": False, "element_bits": 16, "padding": True, "secure": True}, "precompute": {"enable": False}}
    co = FlasheCohort(args, first_idx=0, n_local=2, num_clients=2, prp_seed=R.KEY)
    with pytest.raises(ValueError, match="packed=True"):
        co.decrypt_unquantize(aggregate=np.zeros((4, 2), dtype=np.uint64), packed=True)
    with pytest.raises(ValueError, match="quantize_encrypt first"):
        co.aggregate_packed()
