"""A plain element-wise model of the reference's mask terms, for tests that check single elements of huge vectors.

The CPU oracle fills whole vectors, so it cannot give the expected value of element 2^40 + 3.  This module states the
reference's mask streams (jzf_flashe.py:12-45) one element at a time with Python integers:

    the vector of n elements is cut into n_jobs chunks, the first n % n_jobs of them one element longer than the rest
    (chunks_idx, :12-16); with m = 128 // b elements per AES block, element j of the chunk starting at `begin` is slot
    (j - begin) % m of block i = (j - begin) // m; that block is AES-256 of iter (4 bytes) | idx (4 bytes) | begin + i
    (8 bytes), big-endian, read as a big-endian integer S, and the slot's term is (S >> (b * slot)) mod 2^b.

Everything else (encrypt, decrypt with prefix lists, the sparse single mask of :316-343) is sums of such terms mod 2^b.
Each distinct AES block is computed once (an LRU cache), so a window of a few thousand elements costs a few thousand
host AES calls at most.  The AES is the CPU oracle's (oracle/flashe_oracle.c), not the engine's.
"""
import bisect
import functools

from oracle import flashe_oracle


@functools.lru_cache(maxsize=64)
def chunk_bounds(n, n_jobs):
    """[(begin, end)] of the n_jobs chunks of an n-element vector: sizes d + 1 (the first r) and d, d, r = divmod(n, n_jobs)."""
    d, r = divmod(n, n_jobs)
    out, begin = [], 0
    for c in range(n_jobs):
        size = d + 1 if c < r else d
        out.append((begin, begin + size))
        begin += size
    assert begin == n
    return tuple(out)


def chunk_of(n, n_jobs, j):
    """(begin, end) of the chunk that holds element j."""
    assert 0 <= j < n
    for begin, end in chunk_bounds(n, n_jobs):
        if begin <= j < end:
            return begin, end
    raise AssertionError("unreachable")


@functools.lru_cache(maxsize=1 << 17)
def block(key, it, idx, ctr):
    """S = AES-256(key, iter | idx | ctr) as a big-endian integer."""
    data = it.to_bytes(4, "big") + idx.to_bytes(4, "big") + ctr.to_bytes(8, "big")
    return int.from_bytes(flashe_oracle.aes256_encrypt_block(bytes(key), data), "big")


def term(key, it, idx, n, n_jobs, b, j):
    """Element j's term of the stream (iter, idx) over an n-element vector chunked for n_jobs."""
    begin, _ = chunk_of(n, n_jobs, j)
    m = 128 // b
    i, slot = divmod(j - begin, m)
    S = block(bytes(key), it, idx, begin + i)
    return (S >> (b * slot)) & ((1 << b) - 1)


def mask(key, it, idx_list, n, n_jobs, b, js):
    """sum over idx_list of term(idx, j) mod 2^b, for every j in js."""
    return [sum(term(key, it, i, n, n_jobs, b, j) for i in idx_list) % (1 << b) for j in js]


def encrypt(key, it, idx, double, n, n_jobs, b, js, pt):
    """FlasheCipher.encrypt of pt[k] at element js[k]: pt + term(idx), minus term(idx + 1) under the double mask."""
    out = []
    for j, v in zip(js, pt):
        t = int(v) + term(key, it, idx, n, n_jobs, b, j)
        if double:
            t -= term(key, it, idx + 1, n, n_jobs, b, j)
        out.append(t % (1 << b))
    return out


def decrypt(key, it, add_idx, minus_idx, n, n_jobs, b, js, ct):
    """ct[k] + sum term(add_idx) - sum term(minus_idx) at element js[k], mod 2^b."""
    return [(int(v) + sum(term(key, it, a, n, n_jobs, b, j) for a in add_idx)
             - sum(term(key, it, s, n, n_jobs, b, j) for s in minus_idx)) % (1 << b) for j, v in zip(js, ct)]


def sparse_term(key, it, c, loc, n_jobs, b, p):
    """Client c's single-mask term at dense position p, or None when its strictly increasing list does not hold p: the stream
    of prefix iter | c over the COMPACT positions 0 .. len(loc) - 1 (chunked over len(loc)), the q-th value going to loc[q]."""
    q = bisect.bisect_left(loc, p)
    if q == len(loc) or loc[q] != p:
        return None
    return term(key, it, c, len(loc), n_jobs, b, q)


def sparse_minus_mask(key, it, locs, n_jobs, b, positions):
    """The dense minus-mask of the sparse single-mask decrypt at the given positions: the sum over clients c (position in
    `locs`) of the term c's list puts there, mod 2^b.  Lists must be strictly increasing."""
    locs = [[int(v) for v in l] for l in locs]
    for l in locs:
        assert all(l[i] < l[i + 1] for i in range(len(l) - 1)), "strictly increasing lists only"
    out = []
    for p in positions:
        s = 0
        for c, loc in enumerate(locs):
            t = sparse_term(key, it, c, loc, n_jobs, b, p)
            s += t or 0
        out.append(s % (1 << b))
    return out
