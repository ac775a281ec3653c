"""The CPU oracle's codec against the independent NumPy / Python-int reference of tests/codec_ref.py, over the whole edge plane,
bit for bit (floats compared as bytes).  The oracle is what every GPU codec test is measured against, and its codec is a twin of the
device code: this file is what ties the pair to the reference's own arithmetic."""
import numpy as np
import pytest

import codec_ref as R


def test_the_plane_keeps_what_the_two_rules_allow():
    """6 alphas x 14 widths = 84 cases per dtype.  float64 loses none; float32 loses alpha = 1e30 at every width whose largest image
    2e30 * (2^bits - 1) passes the float32 maximum (3.4e38), i.e. 2^bits > 1.7e8: the 7 widths from 31 up.  Nothing else may go."""
    kept64, dropped64 = R.quantize_cases(np.float64)
    kept32, dropped32 = R.quantize_cases(np.float32)
    assert (len(kept64), dropped64) == (84, 0)
    assert (len(kept32), dropped32) == (77, 7)
    assert all(a == 1e30 and w >= 31 for a in R.ALPHAS for w in R.WIDTHS if (a, w) not in kept32)
    for dt in (np.float32, np.float64):
        for alpha in R.ALPHAS:
            x = R.edge_plane(dt, alpha)
            assert x.dtype == dt and len(x) >= 20000 + 4097 + 17 + 40, len(x)      # fill + line + edges + integer images


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_oracle_quantize_is_the_numpy_expression(oracle, dtype):
    kept, _ = R.quantize_cases(dtype)
    assert len(kept) >= (77 if dtype == np.float32 else 84)
    n_checked = 0
    for alpha in R.ALPHAS:
        x = R.edge_plane(dtype, alpha)
        for bits in [w for a, w in kept if a == alpha]:
            for kind in R.DRAWS:
                u = R.draws(kind, len(x), seed=bits)
                want = R.ref_quantize(x, alpha, bits, u)
                got = oracle.quantize(x, alpha, bits, u)
                bad = np.flatnonzero(got != want.astype(np.uint64))
                assert bad.size == 0, (dtype.__name__, alpha, bits, kind, x[bad[:4]], got[bad[:4]], want[bad[:4]])
                R.check_properties(x, alpha, bits, got, u)
                n_checked += 1
    assert n_checked == 4 * len(kept)


@pytest.mark.parametrize("bits,C", R.PAIRS)
@pytest.mark.parametrize("alpha", [6.5, 8.17121, 1e-30])
def test_oracle_unquantize_is_the_python_int_expression(oracle, bits, C, alpha):
    """Every (bits, C) pair the ABI admits, the ones whose denominator (2^bits - 1) * C passes 2^64 included."""
    for limbs in (1, 2):
        vals = R.sum_plane(bits, C, int_bits=64 * limbs)
        assert len(vals) >= 3000
        if (bits, C) == (62, 5):
            vals.append(0x13ffffffffffffffb if limbs == 2 else 0xfffffffffffffffb)
        want = R.ref_unquantize(vals, alpha, bits, C)
        got = oracle.unquantize(R.to_limbs(vals, limbs), alpha, bits, C)
        bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
        assert got.tobytes() == want.tobytes(), (bits, C, limbs, [hex(vals[i]) for i in bad[:4]], got[bad[:4]], want[bad[:4]])


def test_the_wrapping_example_of_the_denominator(oracle):
    """(2^62 - 1) * 5 needs 65 bits.  On Python ints the value 0x13ffffffffffffffb = 5 * (2^62 - 1) comes back as alpha * C = 32.5."""
    v = [0x13ffffffffffffffb]
    assert R.ref_unquantize(v, 6.5, 62, 5)[0] == 32.5
    assert oracle.unquantize(R.to_limbs(v, 2), 6.5, 62, 5)[0] == 32.5
    assert R.ref_unquantize(v, 6.5, 62, 10)[0] == oracle.unquantize(R.to_limbs(v, 2), 6.5, 62, 10)[0]


@pytest.mark.parametrize("int_bits,field_bits", [(128, 20), (120, 20), (64, 17), (100, 33), (64, 64), (128, 64), (20, 20), (64, 1)])
def test_oracle_batch_and_unbatch_are_the_python_int_expressions(oracle, int_bits, field_bits):
    rng = np.random.RandomState(int_bits + field_bits)
    eb = min(field_bits, 62)
    for n in (1, 2, 5, 6, 7, 1000, 1001, 4097):
        vals = [int.from_bytes(rng.bytes(8), "little") >> (64 - eb) for _ in range(n)]
        vals[0], vals[-1] = (1 << eb) - 1, min(1 << eb, (1 << field_bits) - 1)      # q == 2^bits inside a padded field, where it fits
        want = R.ref_batch(vals, int_bits, field_bits)
        got = oracle.batch(np.array(vals, dtype=np.uint64), int_bits, field_bits)
        assert R.from_limbs(got) == want, (int_bits, field_bits, n)
        back = oracle.unbatch(got, int_bits, field_bits)
        ref_back = R.ref_unbatch(want, int_bits, field_bits)
        assert [int(v) for v in back] == ref_back
        assert ref_back[:n] == vals and not any(ref_back[n:])
    # every field full: the aggregate of num_clients uploads may fill the factor bits too
    L = 2 if int_bits > 64 else 1
    full = [int.from_bytes(rng.bytes(16), "little") % (1 << int_bits) for _ in range(500)] + [(1 << int_bits) - 1, 0]
    assert [int(v) for v in oracle.unbatch(R.to_limbs(full, L), int_bits, field_bits)] == R.ref_unbatch(full, int_bits, field_bits)


def test_ref_shift_and_16_bit_upcasts_are_numpy_and_torch():
    """The helper's own two conventions: `array += scalar` keeps the array's dtype whatever the scalar's type (the loop runs in the
    wider one), and a 16-bit value is computed on as its exact float32 image."""
    x = R.edge_plane(np.float32, 1.0, n_fill=100)
    x = x[np.isfinite(x)]
    narrow, wide = R.ref_shift(x, 0.1), R.ref_shift(x, np.float64(0.1))
    assert narrow.dtype == wide.dtype == np.float32
    assert narrow.tobytes() == (x + np.float32(0.1)).tobytes()
    assert wide.tobytes() == (x.astype(np.float64) + 0.1).astype(np.float32).tobytes()
    assert (narrow != wide).any()                                        # the two loops do differ on this plane
    h = R.edge_plane(np.float32, 1.0, n_fill=100, storage="float16")
    assert h.dtype == np.float32 and (h.astype(np.float16).astype(np.float32) == h).all() and 65504.0 in h
    torch = pytest.importorskip("torch")
    b = R.edge_plane(np.float32, 1.0, n_fill=100, storage="bfloat16")
    assert (torch.from_numpy(b).to(torch.bfloat16).to(torch.float32).numpy() == b).all() and np.isfinite(b[:4]).all()


# ---------------------------------------------------------------------------------------------------------------- cohort cases
def _round_trips(model, bits, b, fb):
    """Per client and row: does ref_unbatch(ref_batch(q)) give q back?"""
    out = []
    for c in range(model.C):
        u = model.u[c * model.n:(c + 1) * model.n]
        for li, (x, row, at) in enumerate(zip(model.ref[c], model.rows, model.starts)):
            q = [int(v) for v in R.ref_quantize(x, row[2], bits, u[at:at + len(x)])]
            out.append((c, li, R.ref_unbatch(R.ref_batch(q, b, fb), b, fb)[:len(q)] == q))
    return out


def test_the_cohort_edge_cases_hold_their_conditions_on_the_reference_alone():
    """Every case of tests/test_gpu_cohort_edges.py, built as the GPU tests build it: no row under overflows() (asserted inside
    check_cohort_case, nothing filtered), a q == 2^bits for every client, a q == 2^bits + 1 wherever a float32 row is quantised to 25 bits
    or more; the batched cases' carries (asserted inside batch_case), told apart by the round trip through ref_unbatch: it gives the
    values back exactly for the rows in which no field overflowed."""
    import test_gpu_cohort_edges as G
    n_cases = 0
    for b, bits in G.COMPACT:
        for J in G.COMPACT_J:
            model, pts = G.compact_case(b, bits, J)
            assert model.n % 2 == 1 and all(s % 2 for s in model.sizes) and len(pts) == G.C == 3
            if bits >= 25:
                assert any((q == (1 << bits) + 1).any() for q in pts)
            n_cases += 1
    for cases, ne in ((G.BATCH_CHAIN, G.CHAIN_ELEMS), (G.BATCH_PREPARED, G.PREPARED_ELEMS)):
        for b, fb, eb in cases:
            model, pts, batched, over = G.batch_case(b, fb, eb, ne)
            bs = b // fb
            assert bs == 1 or ({s % bs for s in model.sizes} >= {0, 1, bs - 1} and 1 in model.sizes and 0 in model.sizes)
            spoilt = {(c, li) for c, li, _e, _s, _ne, _size in over}
            assert bool(spoilt) == (fb == eb)
            for c, li, same in _round_trips(model, eb, b, fb):
                assert same == ((c, li) not in spoilt), (b, fb, eb, c, li)
            if fb == eb and bs * fb == b:
                # the carry out of bit b is what the reduction mod 2^b drops: the unreduced element does not fit b bits
                c, li, e, _s, _ne, _size = next(o for o in over if o[3] == 0)
                u = model.u[c * model.n + model.starts[li]:c * model.n + model.starts[li] + model.sizes[li]]
                q = R.ref_quantize(model.ref[c][li], model.rows[li][2], eb, u)
                assert R.ref_batch(q, b, fb)[e] >> b == 1
            n_cases += 1
    for b, eb, shape in G.SPARSE:
        model, pts, u, zzz, zeros, K, n_jobs = G.sparse_case(b, eb, shape)
        assert model.n == K and len(u) == G.C * (K + 1) and zeros[1] == 1 << eb and zeros[2] == 0
        n_cases += 1
    for b, bits, _compact in G.PREPARED:
        for n in (None, 4097, 4098, 4099) if (b, bits, _compact) in G.PREPARED_TYPES else (None,):
            G.prepared_case(b, bits, n)
            n_cases += 1
    for case in G.BACK_END:
        layers, items, want = G.back_end_case(*case)
        assert len(want) == sum(l[0] for l in layers) and any(l[0] % (case[0] // case[1]) for l in layers)
        n_cases += 1
    assert n_cases == 12 + 5 + 8 + 18 + 7 + 9 + 2
