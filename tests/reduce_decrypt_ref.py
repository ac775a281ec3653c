"""The arbiter's reduce fused with the decrypt of its result, on Python integers:

    agg[j] = sum_c ops[c][j] mod 2^b,        out[j] = (agg[j] + S_add[j] - S_minus[j]) mod 2^b

(`reference`), a host mirror of the geometry that launch_small_reduce_decrypt gives its kernels -- written out here once more, NOT read
from the library, so that a test can name the shape it runs and tests/test_reduce_decrypt_ref_host.py can assert that the shape holds
the edge its name promises -- the shapes themselves (shared by tests/test_gpu_reduce_decrypt_edges.py and the host file), and `Arena`:
operands and outputs laid out between guard zones in one poisoned device block, read back whole and compared with what was uploaded.

THE MIRROR MUST MOVE TOGETHER WITH launch_small_reduce_decrypt, block_of AND grid_for (flashe_amd/csrc/kernels.hip, device_common.h)."""
import numpy as np

KEY = bytes(range(32))
IT, ADD, MINUS = 13, 6, 3           # iteration and the two prefix indices every case uses
WAVES = 16                          # waves of a workgroup: kSmallThreads / 64
WIDE_THREADS = 1024                 # kPrfThreads: reduce_decrypt_ptrs_kernel's grid is grid_for(count, kPrfThreads)
K_SUM_REGS = 10
MAX_OPS = 64                        # kMaxOps


# ------------------------------------------------------------------------------------------------------------------ the reference
def reference(b, ops, add_mask, minus_mask=None):
    """ops: C lists of Python ints (any size: reduced here), masks: lists of Python ints or None -> (agg, out)."""
    mod = 1 << b
    agg = [sum(col) % mod for col in zip(*ops)]
    if minus_mask is None:
        out = [(a + s) % mod for a, s in zip(agg, add_mask)]
    else:
        out = [(a + s - t) % mod for a, s, t in zip(agg, add_mask, minus_mask)]
    return agg, out


def limbs_to_ints(arr):
    arr = np.asarray(arr, dtype=np.uint64)
    if arr.ndim == 1 or arr.shape[1] == 1:
        return [int(x) for x in arr.reshape(-1)]
    return [int(lo) | (int(hi) << 64) for lo, hi in zip(arr[:, 0], arr[:, 1])]


_masks = {}


def mask_ints(oracle, idx, n, J, b):
    """term(IT, idx) of an n-vector in J chunks as Python ints (the oracle's, which tests/golden pins), computed once per shape."""
    key = (idx, n, J, b)
    if key not in _masks:
        _masks[key] = limbs_to_ints(oracle.mask(KEY, IT, idx, n, J, b))
    return _masks[key]


# ------------------------------------------------------------------------------------------------------------------ the geometry
def m_of(b):
    return 128 // b


def tile_blocks(b):
    return 64 if b > 32 else 32


def chunk_bounds(n, J):
    """J chunks, the first n % J of them of n // J + 1 elements."""
    d, r = divmod(n, J)
    out, s = [], 0
    for c in range(J):
        e = s + d + (1 if c < r else 0)
        out.append((s, e))
        s = e
    return out


def blocks_of_vector(n, J, m):
    """[(first element, elements)] of every AES block in the kernels' global numbering: each chunk padded to whole blocks."""
    out = []
    for s, e in chunk_bounds(n, J):
        for j0 in range(s, e, m):
            out.append((j0, min(m, e - j0)))
    return out


def block_of(j, n, J, m):
    """kernels.hip's block_of, the same arithmetic."""
    d, r = divmod(n, J)
    nb1 = (d + 1 + m - 1) // m
    nb0 = (d + m - 1) // m if d else 0
    if j < r * (d + 1):
        c = j // (d + 1)
        return c * nb1 + (j - c * (d + 1)) // m
    j2 = j - r * (d + 1)
    c = j2 // d
    return r * nb1 + c * nb0 + (j2 - c * d) // m


def tiles_of_range(b, n, J, first, count):
    """The tiles of a launch on [first, first + count): lists of (first element, elements) of the T (the last: fewer) blocks each."""
    m, T = m_of(b), tile_blocks(b)
    blocks = blocks_of_vector(n, J, m)
    bf = block_of(first, n, J, m)
    bc = block_of(first + count - 1, n, J, m) - bf + 1
    mine = blocks[bf:bf + bc]
    return [mine[t:t + T] for t in range(0, bc, T)]


def epl_of(b):
    """The E rule of launch_small_reduce_decrypt: among 4, 3, 2 the widths that divide 32 m; the one that fills the most lanes of the
    wave's accesses; ties go to the wider.  -> (E, active lanes of the last trip of the lane loop, trips)"""
    tile = 32 * m_of(b)
    best, best_util = 4, -1.0
    for e in (4, 3, 2):
        if tile % e:
            continue
        lanes = tile // e
        trips = (lanes + 63) // 64
        util = lanes / (64.0 * trips)
        if util > best_util + 1e-9:
            best, best_util = e, util
    lanes = tile // best
    trips = (lanes + 63) // 64
    return best, lanes - 64 * (trips - 1), trips


def is_regular(tile, b, first, count, epl=None):
    """The compact vector path's condition on a tile (the alignment of the pointers aside)."""
    m, T = m_of(b), tile_blocks(b)
    if len(tile) != T or any(cnt < m for _, cnt in tile):
        return False
    e0 = tile[0][0]
    if e0 < first or e0 + T * m > first + count:
        return False
    return epl != 4 or (e0 - first) % 4 == 0


def features(b, n, J, first=0, count=None):
    """What a launch on [first, first + count) of an n-vector in J chunks contains, by the mirror above."""
    count = n - first if count is None else count
    m, T = m_of(b), tile_blocks(b)
    tiles = tiles_of_range(b, n, J, first, count)
    end = first + count
    d = n // J
    f = dict(tiles=len(tiles), d=d, chunk_ends_in_a_tile=0, partial_block=False, whole_tile=False, regular_inside=0, cut_at_start=False,
             cut_at_end=False, regular_declined_by_e4=0, odd_e0t=False, end_one_short=False, one_element_blocks=all(cnt == 1 for t in tiles for _, cnt in t))
    chunk_ends = set(e for s, e in chunk_bounds(n, J) if e > s)
    f["max_tile"] = len(tiles) - 1
    for t in tiles:
        ends = sum(1 for j0, cnt in t if j0 + cnt in chunk_ends)
        f["chunk_ends_in_a_tile"] = max(f["chunk_ends_in_a_tile"], ends)
        f["partial_block"] |= any(cnt < m for _, cnt in t)
        whole = len(t) == T and all(cnt == m for _, cnt in t)
        f["whole_tile"] |= whole
        if whole:
            e0 = t[0][0]
            f["odd_e0t"] |= bool(e0 & 1)
            if is_regular(t, b, first, count):
                f["regular_inside"] += 1
                f["regular_declined_by_e4"] += (e0 - first) % 4 != 0
            f["cut_at_start"] |= e0 < first < e0 + T * m
            f["cut_at_end"] |= e0 < end < e0 + T * m
            f["end_one_short"] |= e0 >= first and e0 + T * m == end + 1          # (what `<= range_end` and `<= range_end + 1` tell apart)
    return f


def straddles_a_word(b):
    """b <= 32: some slot t < m has bits in two 32-bit words of its block."""
    return any((b * t) % 32 + b > 32 for t in range(m_of(b)))


def reads_w2(b):
    """b > 32: some slot starts off a word boundary (sh != 0: the walk reads w[2]) -> (reads it, reads it past word 3 of its row)."""
    offs = [b * t for t in range(m_of(b))]
    return any(o % 32 for o in offs), any(o % 32 and o // 32 + 2 > 3 for o in offs)


# ------------------------------------------------------------------------------------------------------------------ the shapes
ONE_LIMB_WIDTHS = list(range(1, 65))
COMPACT_WIDTHS = list(range(1, 33))


def width_shape(b):
    """1. every width: chunk ends in mid tile, the last block partial, more than two tiles."""
    return (2 * tile_blocks(b) + 5) * m_of(b) + 3, 3


CHUNK_WIDTHS = [64, 40, 33, 32, 20, 8]


def chunk_shapes(b):
    """2. name -> (n, J)"""
    m, T = m_of(b), tile_blocks(b)
    return {
        "more_chunks_than_elements": (5, 16),                # d = 0: five one-element blocks, five chunk ends in the one tile
        "chunk_of_m": (3 * (m - 1) + 1, 3),                   # n // J + 1 == m
        "chunk_of_m_plus_1": (3 * m + 1, 3),                  # n // J + 1 == m + 1
        "chunk_of_2m_minus_1": (3 * (2 * m - 2) + 1, 3),      # n // J + 1 == 2 m - 1
        "one_chunk": (T * m + m + 1, 1),                      # a tile of whole blocks, a whole block, a partial one
        "one_element": (1, 1),
        "one_element_of_three_chunks": (1, 3),
    }


TRIP_WIDTHS = [64, 33, 32, 20, 16]


def trip_shapes(b):
    """3. on one CU (grid = 1): a wave's second trip starts at tile 16.  [(n, J)]"""
    per = WAVES * tile_blocks(b) * m_of(b)
    return [(per - 1, 1), (per, 1), (per + 1, 1), (2 * per + 1, 1), (per + 1, 7)]


VECTOR_WIDTHS = [32, 20, 16, 25, 11]


def vector_shape(b, J):
    """4. about six tiles; J = 3: the second chunk starts at an element = 2 mod 4, the third at one = 0 mod 4."""
    return 6 * 32 * m_of(b) + 5, J


def vector_ranges(b, J):
    """(first, count): first in {0, 4, 8, a tile, a tile -+ 4, a chunk start} x an end on a tile boundary, 4, 2 and 1 short of it, 1 past it, the vector's."""
    n, _ = vector_shape(b, J)
    tile = 32 * m_of(b)
    start = chunk_bounds(n, J)[1][0] if J > 1 else 0
    firsts = [0, 4, 8, tile, tile - 4, tile + 4, start, 2, tile + 2]    # (2: inside a block at every m, m = 4 included)
    if J > 1:
        # the tile boundaries of the later chunks follow the chunk's start
        ends = [start + 2 * tile, start + 2 * tile - 4, start + 2 * tile - 2, start + 2 * tile - 1, start + 2 * tile + 1, n]
    else:
        ends = [5 * tile, 5 * tile - 4, 5 * tile - 2, 5 * tile - 1, 5 * tile + 1, n]      # (2 and 1 short: inside the tile's last block at m = 4 too)
    return sorted(set((f, e - f) for f in firsts for e in ends if e > f))


OPERAND_COUNTS = [1, 2, 3, 7, 8, 9, 16, 17, 63, 64]
WIDE_OPERAND_COUNTS = [1, 9, 10, 11, 64]
WRAP_SMALL = [32, 31, 64, 63, 33]
WRAP_WIDE = [128, 127, 65]
WIDE_WIDTHS = [65, 100, 128]


def wide_second_trip(num_cus):
    """8. reduce_decrypt_ptrs_kernel: grid = grid_for(count, kPrfThreads) = min(ceil(count / 1024), num_cus) workgroups of 1024 lanes,
    one element per lane and trip: the first count at which a lane makes a second trip."""
    return num_cus * WIDE_THREADS + 1


# ------------------------------------------------------------------------------------------------------------------ the guarded block
POISON = 0xC7
GUARD = 512


class Arena:
    """Vectors between guard zones in ONE poisoned device block.  add() reserves, commit() uploads the image, fetch() reads the block
    back and asserts that every byte outside the outputs -- the guards on both sides of each vector, the operands -- is what was uploaded.
    `shift`: bytes past a 16-byte boundary at which the vector begins."""

    def __init__(self, eng):
        self.eng, self.size, self.reg, self.buf, self.after = eng, GUARD, {}, None, None

    def add(self, name, nbytes, data=None, shift=0):
        off = (self.size + 15) // 16 * 16 + shift
        self.reg[name] = (off, int(nbytes), None if data is None else np.ascontiguousarray(data).view(np.uint8).reshape(-1))
        self.size = off + int(nbytes) + GUARD
        return self

    def commit(self):
        self.image = np.full(self.size + 16, POISON, dtype=np.uint8)
        for off, nbytes, data in self.reg.values():
            if data is not None:
                assert data.nbytes == nbytes
                self.image[off:off + nbytes] = data
        self.buf = self.eng.alloc(self.image.nbytes)
        self.buf.upload(self.image)
        return self

    def ptr(self, name):
        return self.buf.ptr + self.reg[name][0]

    def fetch(self):
        self.after = self.buf.download(np.uint8)
        keep = np.ones(self.image.nbytes, dtype=bool)
        for off, nbytes, data in self.reg.values():
            if data is None:
                keep[off:off + nbytes] = False
        bad = np.flatnonzero((self.after != self.image) & keep)
        assert bad.size == 0, ("bytes outside the outputs were written", [int(x) for x in bad[:8]], self.where(int(bad[0])) if bad.size else None)
        return self

    def where(self, pos):
        for name, (off, nbytes, _) in self.reg.items():
            if off - GUARD <= pos < off + nbytes + GUARD:
                return name, pos - off
        return None

    def untouched(self, name):
        off, nbytes, _ = self.reg[name]
        return bool((self.after[off:off + nbytes] == POISON).all())

    def values(self, name, elem):
        """The output `name` as Python ints (elem = 4, 8 or 16 bytes per element)."""
        off, nbytes, _ = self.reg[name]
        raw = self.after[off:off + nbytes].copy()
        if elem == 4:
            return [int(x) for x in raw.view(np.uint32)]
        w = raw.view(np.uint64)
        if elem == 8:
            return [int(x) for x in w]
        return [int(lo) | (int(hi) << 64) for lo, hi in zip(w[0::2], w[1::2])]

    def free(self):
        if self.buf is not None:
            self.buf.free()
            self.buf = None


def to_array(vals, elem):
    """Python ints -> the array an operand of `elem` bytes per element is uploaded as."""
    if elem == 4:
        return np.array(vals, dtype=np.uint32)
    if elem == 8:
        return np.array(vals, dtype=np.uint64)
    out = np.zeros((len(vals), 2), dtype=np.uint64)
    for k, v in enumerate(vals):
        out[k, 0] = v & (2 ** 64 - 1)
        out[k, 1] = v >> 64
    return out
