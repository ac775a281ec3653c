"""What the GPU tests of the packed wire kernels (wire.hip) share: the models they feed, the expected wire integer and floats, and the
round trip through flashe_quantize_encrypt_pack_tensors_dev / flashe_unpack_decrypt_unquantize_model_dev (a plain helper, no conftest).

No kernel of the engine goes into an expected value.  Way out: the Python int sum(ct[j] << (b * (n - 1 - j))) (jzf_weights.py
`_to_bytes_old`), ct = the CPU oracle's encrypt of the plaintexts tests/codec_ref.py quantises, masked to b bits.  Way back: float64 BYTES
against codec_ref's unquantise of the oracle's decrypt.  A guard limb / guard value lies past each output.

tiles() restates the kernels' tiling -- chunks_idx(range(n), n_jobs) cut into blocks of m = 128 // b elements, 64 blocks to a tile -- so that
a test can assert, on its inputs alone, that a shape reaches the path it is there for."""
import functools

import numpy as np

import codec_ref as R

KEY = bytes(range(32))
IT, IDX, EBITS, C = 9, 4, 12, 3
ALPHAS = (8.17121, 3e-3, 6.5)
GUARD = (1 << 64) - 1


def wire_int(ct, b):
    """sum(ct[j] << (b * (n - 1 - j))), 256 elements at a time (the one-by-one sum is quadratic in n)."""
    acc = 0
    for at in range(0, len(ct), 256):
        part = 0
        for v in ct[at:at + 256]:
            part = (part << b) | int(v)
        acc = (acc << (b * len(ct[at:at + 256]))) | part
    return acc


def n_limbs_of(n, b):
    return (n * b + 63) // 64


def int_limbs(v, n_limbs):
    """The little-endian 64-bit limbs of a wire integer: limb i = bits [64 i, 64 i + 64)."""
    return np.frombuffer(int(v).to_bytes(8 * n_limbs, "little"), dtype=np.uint64)


def tiles(n, n_jobs, m):
    """(e0, e1, ragged) of every tile of an n-vector cut into n_jobs chunks (the first n % n_jobs one element longer), each chunk into
    blocks of m elements (its last one may hold fewer), 64 consecutive blocks to a tile.  ragged: the tile holds a partial block.  A tile
    that is not ragged covers exactly the elements [e0, e1)."""
    d, r = divmod(n, n_jobs)
    blocks, begin = [], 0
    for c in range(n_jobs):
        size = d + 1 if c < r else d
        blocks += [(begin + i, min(m, size - i)) for i in range(0, size, m)]
        begin += size
    out = []
    for t in range(0, len(blocks), 64):
        tb = blocks[t:t + 64]
        out.append((tb[0][0], tb[-1][0] + tb[-1][1], any(cnt < m for _j0, cnt in tb)))
    return out


def whole_tiles_in(n, n_jobs, m, lo, hi):
    """The tiles without a partial block that lie inside the elements [lo, hi): the ones the kernels take a row at a time."""
    return [(e0, e1) for e0, e1, ragged in tiles(n, n_jobs, m) if not ragged and lo <= e0 and e1 <= hi]


class WireModel:
    """A flattened model of n values in rows: sizes, starts, alphas; held[l] = what lies in device memory (float arrays, uint16 patterns
    for the 16-bit formats), codes[l] / shifts[l] / flags[l] = the row's flashe_tensor_layer dtype code, shift and flags; ref[l] = the
    compute-type array the codec quantises (upcast, shifted, widened); u = the n draws."""

    def __init__(self, sizes, alphas, held, codes, shifts, flags, ref, u):
        self.sizes, self.alphas, self.held, self.codes, self.shifts, self.flags, self.ref, self.u = (
            tuple(int(s) for s in sizes), tuple(alphas), list(held), tuple(codes), tuple(shifts), tuple(flags), list(ref), u)
        self.starts = tuple(int(v) for v in np.concatenate([[0], np.cumsum(self.sizes)[:-1]]))
        self.n = int(sum(self.sizes))
        assert len(u) == self.n and all(len(x) == s == len(h) for x, s, h in zip(self.ref, self.sizes, self.held))


@functools.lru_cache(maxsize=None)
def three_layer_model(n):
    """n values in three direct rows -- float64 of min(7, n // 2) values, two float32 -- with ALPHAS, filled by layer_fill, under
    mixed_draws.  Shared between the tests that ask for the same n: nobody writes to it."""
    s0 = min(7, max(1, n // 2))
    s1 = (n - s0) // 2
    sizes, dts = (s0, s1, n - s0 - s1), (np.float64, np.float32, np.float32)
    xs = [R.layer_fill(dt, a, s, seed=l) if s else np.zeros(0, dt) for l, (dt, a, s) in enumerate(zip(dts, ALPHAS, sizes))]
    return WireModel(sizes, ALPHAS, xs, [R.F64 if dt == np.float64 else R.F32 for dt in dts], [0.0] * 3, [0] * 3, xs, R.mixed_draws(n))


def cohort_wire_model(spec, seed=0):
    """The one-client codec_ref.cohort_model of `spec` -- rows of (storage, alpha, shift, wide, loop64, size) -- as a WireModel: the rows
    carry the STORAGE dtype code, as the tensor entry points take them, and the plaintexts come from model.ref[0]."""
    m = R.cohort_model(spec, 1, seed)
    return WireModel(m.sizes, [row[2] for row in m.rows], m.storage[0], m.dts, [row[3] for row in m.rows], [row[5] for row in m.rows], m.ref[0], m.u)


def own_mask(scheme):
    """(add, minus): the prefix lists that undo one client's own mask."""
    return ([IDX + 1], [IDX]) if scheme == "double" else ([], [IDX])


def row_floats(values, starts, sizes, alphas, ebits=EBITS, num_clients=C):
    """codec_ref's unquantise of decrypted elements (Python ints), every row with its own alpha."""
    parts = [R.ref_unquantize(values[s:s + sz], a, ebits, num_clients) for s, sz, a in zip(starts, sizes, alphas) if sz]
    return np.concatenate(parts + [np.zeros(0)])


def expected(orc, model, b, scheme, n_jobs):
    """(the wire integer of the client's upload, add, minus, the floats the same integer decrypts and unquantises to)."""
    q = np.concatenate([R.ref_quantize(x, a, EBITS, model.u[s:s + len(x)]) for x, a, s in zip(model.ref, model.alphas, model.starts) if len(x)])
    pt = (q.astype(np.uint64) & np.uint64((1 << b) - 1))
    ct = orc.limbs_to_ints(orc.encrypt(KEY, IT, IDX, scheme, n_jobs, b, pt))
    add, minus = own_mask(scheme)
    dec = orc.limbs_to_ints(orc.decrypt(KEY, IT, add, minus, n_jobs, b, orc.ints_to_limbs(ct, b)))
    return wire_int(ct, b), add, minus, row_floats(dec, model.starts, model.sizes, model.alphas)


def check_way_out(eng, model, b, scheme, n_jobs, want, tag):
    from flashe_amd.engine import SCHEME_DOUBLE, SCHEME_SINGLE
    n, n_limbs = model.n, n_limbs_of(model.n, b)
    bufs = [eng.upload(x) if len(x) else None for x in model.held]
    rows = [(s, buf.ptr if buf else None, a, sh, code, fl)
            for s, buf, a, sh, code, fl in zip(model.starts, bufs, model.alphas, model.shifts, model.codes, model.flags)]
    packed = eng.alloc(8 * (n_limbs + 1))
    eng.memset_dev(packed, 0xFF, packed.nbytes)
    assert eng.quantize_encrypt_pack_tensors_dev(IT, IDX, SCHEME_DOUBLE if scheme == "double" else SCHEME_SINGLE, n, n_jobs, rows, EBITS, eng.upload(model.u), packed)
    got = packed.download(np.uint64, n_limbs + 1)
    assert int(got[n_limbs]) == GUARD, ("guard limb",) + tag
    assert int.from_bytes(got[:n_limbs].tobytes(), "little") == want, ("way out",) + tag + (np.flatnonzero(got[:n_limbs] != int_limbs(want, n_limbs))[:4],)


def check_way_back(eng, big, n, b, add, minus, n_jobs, starts, alphas, floats, tag, ebits=EBITS, num_clients=C):
    """The wire integer `big` through the unpack entry point: float64 bytes against `floats`, the guard value behind them untouched."""
    n_limbs = n_limbs_of(n, b)
    out = eng.alloc(8 * (n + 1))
    eng.memset_dev(out, 0xFF, out.nbytes)
    din = eng.upload(int_limbs(big, n_limbs))
    back = [(int(s), None, a, False) for s, a in zip(starts, alphas)]
    assert eng.unpack_decrypt_unquantize_model_dev(IT, add, minus, n, n_jobs, din, back, ebits, num_clients, out)
    res = out.download(np.uint64, n + 1)
    assert int(res[n]) == GUARD, ("guard value",) + tag
    assert res[:n].tobytes() == floats.tobytes(), ("way back",) + tag + (np.flatnonzero(res[:n] != floats.view(np.uint64))[:4],)


def round_trip(eng, orc, b, scheme, n_jobs, model):
    """Both directions of one model: the packed limbs against the Python int, then that integer itself back to the floats."""
    tag = (b, scheme, n_jobs, model.n)
    want, add, minus, floats = expected(orc, model, b, scheme, n_jobs)
    check_way_out(eng, model, b, scheme, n_jobs, want, tag)
    check_way_back(eng, want, model.n, b, add, minus, n_jobs, model.starts, model.alphas, floats, tag)
