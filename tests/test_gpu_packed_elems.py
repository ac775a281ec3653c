"""GPU: the arbiter's packed reduce computed on UNPACKED ciphertext vectors --

    aggregate_packed_elems_kernel<0 | 1 | 2>      (uint32 elements; one uint64 limb; two limbs) + packed_elems_fixup_kernel
    aggregate_packed_elems_u32x4_kernel           (uint32 elements, every pointer 16-byte aligned: four per lane)

through Engine.aggregate_packed_elems_dev / aggregate_packed_elems_u32_dev, and through FlasheCohort.aggregate_packed() and
decrypt_unquantize(packed=True).  Every value is compared exactly with tests/packed_elems_ref.py (Python big integers: pack, add, unpack);
operands and the output lie between guard zones in one poisoned block that is read back whole, so a store outside the output or into an
operand fails the case.  The shapes come from packed_elems_ref.py, where tests/test_packed_elems_ref_host.py asserts without a GPU that
each one holds the edge it is named after."""
import numpy as np
import pytest

import packed_elems_ref as R
from reduce_decrypt_ref import Arena

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    from flashe_amd import engine as E
    cache = {}

    def get(b, one_cu=False):
        if (b, one_cu) not in cache:
            e = E.Engine(R.KEY, b, device=0)
            if one_cu:
                e.set_cu_limit(1)
            cache[b, one_cu] = e
        return cache[b, one_cu]

    yield get
    for e in cache.values():
        e.close()


_REF = {}


def _want(b, ops, key):
    """The reference of a named case, computed once."""
    if key not in _REF:
        _REF[key] = R.reference(b, ops)
    return _REF[key]


def _same(got, want, ctx):
    if got != want:
        bad = [k for k, (g, w) in enumerate(zip(got, want)) if g != w]
        pytest.fail("%r: %d of %d elements differ, the first at %d: got %#x, want %#x" % (ctx, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]]))


def run(eng, b, ops, key, compact=False, shift=None, separate=False):
    """One call on operands laid out in a guarded block (or in allocations of their own), compared with the reference."""
    eb, n, C, shift = R.elem_bytes(b, compact), len(ops[0]), len(ops), shift or {}
    ctx = dict(b=b, n=n, C=C, eb=eb, key=key, shift=shift, separate=separate)
    a, held = Arena(eng), []
    try:
        arrs, uniq = [], {}
        for o in ops:                                   # (a pattern may pass one list several times: converted once)
            if id(o) not in uniq:
                uniq[id(o)] = R.to_array(o, eb)
            arrs.append(uniq[id(o)])
        for c in range(C):
            if separate:
                held.append(eng.upload(arrs[c]))
            else:
                a.add("op%d" % c, n * eb, arrs[c], shift.get("op%d" % c, 0))
        a.add("out", n * eb, None, shift.get("out", 0)).commit()
        ptrs = [h.ptr for h in held] if separate else [a.ptr("op%d" % c) for c in range(C)]
        call = eng.aggregate_packed_elems_u32_dev if compact else eng.aggregate_packed_elems_dev
        assert call(ptrs, n, a.ptr("out")) is True, ctx
        _same(a.fetch().values("out", eb), _want(b, ops, key), ctx)
    finally:
        a.free()
        for h in held:
            h.free()


FORMS = [(b, False) for b in R.WIDTHS_U64] + [(b, True) for b in R.WIDTHS_U32]
_id = lambda f: "%d%s" % (f[0], "-u32" if f[1] else "")     # noqa: E731


@pytest.mark.parametrize("form", [(20, True), (20, False), (64, False), (122, False), (128, False)], ids=_id)
def test_lengths_around_a_wave_and_a_block(engines, form):
    b, compact = form
    for n in R.LENGTHS:
        # (compact and aligned is the vector kernel's: one operand 4 bytes off keeps the one-element-per-lane kernel under test)
        off = {"op0": 4} if compact else None
        run(engines(b), b, R.random_ops(b, n, 3, compact), ("len", b, compact, n), compact, shift=off)
        run(engines(b), b, R.all_ones(b, n, 3), ("len-ones", b, n), compact, shift=off)
    for n in (R.LENGTHS_X4 if compact else []):
        run(engines(b), b, R.random_ops(b, n, 3, compact), ("len", b, compact, n), compact)
        run(engines(b), b, R.all_ones(b, n, 3), ("len-ones", b, n), compact)


@pytest.mark.parametrize("form", FORMS, ids=_id)
def test_every_width_and_pattern_over_six_blocks(engines, form):
    b, compact = form
    for name, ops in R.patterns(b, compact=compact).items():
        run(engines(b), b, ops, (name, b, compact), compact, shift={"op1": 12, "out": 8} if compact else None)
    if compact:         # the vector kernel: the same edges of its own blocks and waves
        for name, ops in R.patterns(b, R.N_PATTERN_X4, compact=True, x4=True).items():
            run(engines(b), b, ops, (name, b, "x4"), compact)


@pytest.mark.parametrize("C", R.OPERAND_COUNTS + [2 * R.MAX_OPS + 2])
def test_operand_counts(engines, C):
    """65: two passes through the ctx scratch; 130: three, both scratch vectors.  All ones: h = C - 1 (mod what a pass holds)."""
    n = 2 * R.TILE + 1
    run(engines(20), 20, R.random_ops(20, n, C, True, seed=1), ("count-off", C), True, shift={"op0": 8, "out": 4})
    run(engines(20), 20, R.random_ops(20, 2 * R.TILE_X4 + 1, C, True), ("count-x4", C), True, separate=C > 10)
    for b, compact in ((20, True), (8, False), (64, False), (122, False), (128, False)):
        run(engines(b), b, R.random_ops(b, n, C, compact), ("count", b, compact, C), compact, separate=C > 10)
        ones = [[(1 << b) - 1] * n] * C
        run(engines(b), b, ones, ("count-ones", b, C), compact)


def test_alignments_the_elementwise_twins_accept(engines):
    """One-limb vectors anywhere on 8 bytes, two-limb operands 8 bytes off (out stays 16-byte aligned), uint32 vectors anywhere on 4
    bytes; equally spaced in one block and in allocations of their own."""
    n = R.TILE + 1
    for b, compact, shifts in ((20, True, [{"op0": 4}, {"op1": 8, "out": 12}, {"op0": 12, "op1": 4, "op2": 8, "out": 4}]),
                               (40, False, [{"op1": 8}, {"out": 8}, {"op0": 8, "op1": 8, "op2": 8, "out": 8}]),
                               (128, False, [{"op0": 8}, {"op2": 8}, {"op0": 8, "op1": 8, "op2": 8}]),
                               (100, False, [{"op1": 8}])):
        ops = R.random_ops(b, n, 3, compact)
        for s in shifts:
            run(engines(b), b, ops, ("align", b, compact), compact, shift=s)
        run(engines(b), b, ops, ("align", b, compact), compact, separate=True)


def test_refusals_leave_the_output_untouched(engines):
    from flashe_amd._lib import FlasheError
    # out is one of the operands
    for b, compact in ((20, True), (20, False), (128, False)):
        eng, eb, n = engines(b), R.elem_bytes(b, compact), 300
        ops = R.random_ops(b, n, 2, compact)
        a = Arena(eng)
        try:
            for c in range(2):
                a.add("op%d" % c, n * eb, R.to_array(ops[c], eb))
            a.commit()
            call = eng.aggregate_packed_elems_u32_dev if compact else eng.aggregate_packed_elems_dev
            with pytest.raises(FlasheError):
                call([a.ptr("op0"), a.ptr("op1")], n, a.ptr("op1"))
            eng.sync()
            a.fetch()
        finally:
            a.free()
    # b = 4: sixteen operands are a one-bit carry, seventeen are not -- declined, nothing launched
    eng, n = engines(4), 2 * R.TILE + 1
    run(eng, 4, R.all_ones(4, n, 16), ("b4-ones", 16))
    run(eng, 4, R.random_ops(4, n, 16), ("b4", 16))
    for compact in (False, True):
        eb = R.elem_bytes(4, compact)
        a = Arena(eng)
        try:
            a.add("op", n * eb, R.to_array([15] * n, eb)).add("out", n * eb).commit()
            call = eng.aggregate_packed_elems_u32_dev if compact else eng.aggregate_packed_elems_dev
            assert call([a.ptr("op")] * 17, n, a.ptr("out")) is False
            eng.sync()
            assert a.fetch().untouched("out")
        finally:
            a.free()
    # nothing to do
    assert engines(20).aggregate_packed_elems_dev([engines(20).alloc(16)], 0, None) is True


@pytest.mark.parametrize("form", [(20, True), (64, False), (128, False)], ids=_id)
def test_many_blocks_on_one_compute_unit(engines, form):
    b, compact = form
    eng = engines(b, one_cu=True)
    for name in ("random", "ripple-stop", "all-ones"):
        run(eng, b, R.patterns(b, compact=compact)[name], (name, b, compact), compact, shift={"op0": 4} if compact else None)
        if compact:
            run(eng, b, R.patterns(b, R.N_PATTERN_X4, compact=True, x4=True)[name], (name, b, "x4"), compact)


# ------------------------------------------------------------------------------------------------------------------ class level
class _W:
    def __init__(self, layers):
        self.walking_order = sorted(layers)
        self._weights = dict(layers)


def _args(b):
    return {"quantize": {"int_bits": b, "batch": False, "element_bits": 16, "padding": True, "secure": True}, "precompute": {"enable": False}}


@pytest.mark.parametrize("present", [None, [0, 2]])
@pytest.mark.parametrize("setting", [(128, False, False), (128, False, True), (20, True, False)], ids=["128", "128-cut", "20-compact"])
def test_a_cohort_round_reduced_as_the_dense_jobs_arbiter_reduces_it(setting, present):
    """Three clients, a model of a few thousand values: aggregate_packed() is cipher.aggregate(packed=True) of the clients' own
    FlasheClient ciphertexts, decrypt_unquantize(packed=True) the lead FlasheClient's decrypt of that aggregate bit for bit -- and not
    the decrypt of the element-wise sum."""
    from flashe_amd import cipher as cm
    from flashe_amd.block import FlasheClient, FlasheCohort
    b, compact, cut = setting
    cm.N_JOBS = 16
    C, sizes = 3, [1, 1019, 0, 2048, 777]
    pos = list(range(C)) if present is None else present
    g = np.random.Generator(np.random.PCG64(b))
    models = [{"l%d" % i: (g.standard_normal(s) * 0.05 + 0.01 * c).astype(np.float32 if i % 2 else np.float64) for i, s in enumerate(sizes)} for c in range(C)]
    clients = []
    for c in range(C):
        cl = FlasheClient(_args(b))
        cl.create_cipher(c, C, R.KEY)
        cl.set_iter_index(3)
        clients.append(cl)
    co = FlasheCohort(_args(b), first_idx=0, n_local=C, num_clients=C, prp_seed=R.KEY, compact=compact, cut=cut)
    co.set_iter_index(3)
    np.random.seed(11)
    state = np.random.get_state()
    want_cts = []
    for p in pos:
        w = clients[p].quantize_encrypt(_W(dict(models[p])), device=True)
        want_cts.append(w._weights[w.walking_order[0]])
    want_packed = clients[pos[0]].cipher.aggregate(want_cts, packed=True)
    want_elem = clients[pos[0]].cipher.aggregate(want_cts)
    clients[pos[0]].set_idx_list(list(pos))
    ref = clients[pos[0]].decrypt_unquantize(_W({"l0": want_packed}))
    np.random.set_state(state)
    up = co.quantize_encrypt([_W(dict(models[p])) for p in pos], **({} if present is None else {"present": present}))
    if cut and present is None:
        assert up.path == "cut-chain" and co.lead._cohort_mask is not None       # (so the mask pass below is really exercised)
    got_packed = co.aggregate_packed()
    assert got_packed.compact == compact and len(got_packed) == sum(sizes)
    assert got_packed.to_host().astype(np.uint64).tobytes() == want_packed.to_host().astype(np.uint64).tobytes()
    assert co.aggregate_packed(up).to_host().tobytes() == got_packed.to_host().tobytes()
    # ... and it is the reference's big-integer sum of those ciphertexts, not the element-wise one
    ints = [R.limbs_to_ints(ct.to_host().astype(np.uint64).reshape(len(ct), -1)) for ct in up.ciphertexts]
    assert R.limbs_to_ints(got_packed.to_host().astype(np.uint64).reshape(len(got_packed), -1)) == R.reference(b, ints)
    assert up.partial_sum.to_host().astype(np.uint64).tobytes() == want_elem.to_host().astype(np.uint64).tobytes() != got_packed.to_host().astype(np.uint64).tobytes()
    eng = co.cipher.engine
    kept, seen = co.lead._cohort_mask is not None, []
    for name in ("combine_unquantize_model_dev", "decrypt_unquantize_model_dev", "decrypt_dev"):
        def wrap(fn=getattr(eng, name), name=name):
            def call(*a, **kw):
                seen.append(name)
                return fn(*a, **kw)
            return call
        setattr(eng, name, wrap())
    try:
        got = co.decrypt_unquantize(packed=True)
    finally:
        for name in ("combine_unquantize_model_dev", "decrypt_unquantize_model_dev", "decrypt_dev"):
            delattr(eng, name)
    if kept:        # the launch wrote the decrypt mask: one combine pass, no PRF launch
        assert seen == ["combine_unquantize_model_dev"], seen
    assert (co.lead._cohort_mask is not None) == kept
    plain = co.decrypt_unquantize()
    assert got.walking_order == ref.walking_order
    differ = 0
    for k in ref.walking_order:
        x, y, z = (np.asarray(w._weights[k], dtype=np.float64) for w in (got, ref, plain))
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k
        differ += int((x != z).sum())
    assert differ > 0, "the packed carries must show in the decrypted model"
