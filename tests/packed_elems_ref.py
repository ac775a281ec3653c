"""The arbiter's packed reduce of UNPACKED ciphertext vectors (flashe_aggregate_packed_elems_dev / _u32_dev) in Python integers, and the
shapes tests/test_gpu_packed_elems.py runs.

reference():  the definition -- big-integer pack (element j of n at bit (n - 1 - j) b, masked to b bits: jzf_weights.py:155-195), add
              mod 2^(n b) (jzf_aggregator.py:406-419), unpack.
recurrence(): the same sum in the element domain, as the kernels compute it: column sums S_j = h_j 2^b + s_j, t_j = s_j + h_{j+1},
              g_j = t_j > M, p_j = t_j == M, a one-bit carry k_j = g_j | (p_j & k_{j+1}) from element n - 1 towards element 0, out_j =
              (t_j + k_{j+1}) & M.  Valid while the operands number at most 2^b.
A kernel block owns TILE consecutive RANKS e = n - 1 - j (rank 0 = element n - 1, the least significant), a wave WAVE of them.
The compact layout's vector kernel (every pointer 16-byte aligned) holds four elements per lane: TILE_X4 ranks per block, WAVE_X4 per wave,
counted from the length padded to a multiple of four -- pad_x4(n) virtual zero elements lie under element n - 1.
tests/test_packed_elems_ref_host.py checks both against the oracle and a golden round and that each named shape holds its edge."""
import numpy as np

KEY = bytes(range(32))
TILE, WAVE, MAX_OPS = 256, 64, 64

LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 2 * 256 + 1, 5 * 256 + 3]
OPERAND_COUNTS = [1, 2, 10, 64, 65]
WIDTHS_U64 = [8, 16, 20, 32, 33, 63, 64, 65, 120, 122, 127, 128]
WIDTHS_U32 = [16, 20, 23, 24, 32]
N_PATTERN = 5 * 256 + 3             # six blocks, the last one of three elements
STOP_RANK = 2 * 256 + 88            # in the middle block of N_PATTERN's first five
TILE_X4, WAVE_X4 = 4 * TILE, 4 * WAVE
LENGTHS_X4 = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2 * 1024 + 1, 5 * 1024 + 3]
N_PATTERN_X4 = 5 * 1024 + 3         # six blocks of the vector kernel; one virtual element under the last


def pad_x4(n):
    return -n % 4


def elem_bytes(b, compact=False):
    return 4 if compact else 16 if b > 64 else 8


def pack_int(vals, b):
    M, n, x = (1 << b) - 1, len(vals), 0
    for j, v in enumerate(vals):
        x |= (v & M) << ((n - 1 - j) * b)
    return x


def unpack_int(x, n, b):
    M = (1 << b) - 1
    return [(x >> ((n - 1 - j) * b)) & M for j in range(n)]


def reference(b, ops):
    n = len(ops[0])
    return unpack_int(sum(pack_int(o, b) for o in ops) % (1 << (n * b)), n, b)


def recurrence(b, ops):
    """(out, h, g, p): the element-domain form and its per-element high parts and carry flags (index = element j)."""
    n, C, M = len(ops[0]), len(ops), (1 << b) - 1
    assert C <= (1 << b), "the carry between elements is one bit only while the operands number at most 2^b"
    S = [sum(o[j] & M for o in ops) for j in range(n)]
    s, h = [x & M for x in S], [x >> b for x in S]
    assert all(x <= C - 1 for x in h)
    t = [s[j] + (h[j + 1] if j + 1 < n else 0) for j in range(n)]
    g, p = [x > M for x in t], [x == M for x in t]
    out, k = [0] * n, 0
    for j in range(n - 1, -1, -1):
        assert t[j] + k < (1 << (b + 1))
        out[j] = (t[j] + k) & M
        k = int(g[j] or (p[j] and k))
    return out, h, g, p


def block_summaries(g, p, tile=TILE, pad=0):
    """(G, P) of every block of `tile` ranks with carry-in 0, least significant block first.  pad: virtual zero elements under element
    n - 1 (they neither generate nor propagate), counted as the first ranks."""
    n, res = len(g), []
    for e0 in range(0, n + pad, tile):
        k, allp = 0, True
        for e in range(e0, min(e0 + tile, n + pad)):
            j = n + pad - 1 - e
            gj, pj = (g[j], p[j]) if j < n else (False, False)
            k = int(gj or (pj and k))
            allp = allp and pj
        res.append((k, int(allp)))
    return res


# ------------------------------------------------------------------------------------------------------------------ operand patterns
def by_rank(n, ranks):
    """A vector given by rank (rank e = element n - 1 - e) as a list by element."""
    return [ranks[n - 1 - j] for j in range(n)]


def random_ops(b, n, C, compact=False, seed=0):
    """Random over the whole CONTAINER: at b below the container's width the bits above b must be masked."""
    eb = elem_bytes(b, compact)
    rng = np.random.Generator(np.random.PCG64([b, n, C, eb, seed]))
    out = []
    for _ in range(C):
        raw = np.frombuffer(rng.bytes(n * eb), dtype=np.uint8)
        if eb == 4:
            out.append([int(x) for x in raw.view(np.uint32)])
        else:
            w = [int(x) for x in raw.view(np.uint64)]
            out.append(w if eb == 8 else [lo | (hi << 64) for lo, hi in zip(w[0::2], w[1::2])])
    return out


def all_ones(b, n, C):
    """Every operand M everywhere: h = C - 1 in every column, across every wave and block edge."""
    return [[(1 << b) - 1] * n for _ in range(C)]


def ripple_out(b, n):
    """One operand all M plus a 1 in the last element: the carry ripples through the whole vector and out of element 0; all zeros."""
    return [[(1 << b) - 1] * n, [0] * (n - 1) + [1]]


def ripple_stop(b, n, stop_rank=STOP_RANK):
    """ripple_out with the element of rank stop_rank set to M - 1: the ripple stops there.  Its block's carry-in comes from a generating
    block behind a fully propagating one."""
    a, one = ripple_out(b, n)
    a[n - 1 - stop_rank] = (1 << b) - 2
    return [a, one]


def chain_to(b, n, end_rank, fill=5):
    """A carry generated at rank 0 that propagates through ranks 1 .. end_rank - 1 and is absorbed at rank end_rank."""
    M = (1 << b) - 1
    return [by_rank(n, [M if e < end_rank else fill for e in range(n)]), by_rank(n, [1 if e == 0 else 0 for e in range(n)])]


def patterns(b, n=N_PATTERN, compact=False, x4=False):
    """name -> operands: the patterns every width runs at n = N_PATTERN; x4: the same edges of the vector kernel's blocks and waves
    (n = N_PATTERN_X4), whose ranks count from the padded length."""
    tile, wave, pad = (TILE_X4, WAVE_X4, pad_x4(n)) if x4 else (TILE, WAVE, 0)
    return {"random": random_ops(b, n, 10, compact), "all-ones": all_ones(b, n, 10), "ripple-out": ripple_out(b, n),
            "ripple-stop": ripple_stop(b, n, 2 * tile + 88 - pad), "chain-past-wave": chain_to(b, n, wave - pad),
            "chain-past-block": chain_to(b, n, tile - pad)}


# ------------------------------------------------------------------------------------------------------------------ upload helpers
def limbs_to_ints(arr):
    """A uint64 array [n, L] as Python ints."""
    a = np.asarray(arr, dtype=np.uint64).reshape(len(arr), -1)
    return [int(r[0]) | ((int(r[1]) << 64) if a.shape[1] == 2 else 0) for r in a]


def to_array(vals, eb):
    """Python ints -> the array an operand of `eb` bytes per element is uploaded as."""
    if eb == 4:
        return np.array(vals, dtype=np.uint32)
    if eb == 8:
        return np.array(vals, dtype=np.uint64)
    out = np.zeros((len(vals), 2), dtype=np.uint64)
    for k, v in enumerate(vals):
        out[k, 0] = v & (2 ** 64 - 1)
        out[k, 1] = v >> 64
    return out
