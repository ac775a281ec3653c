"""GPU: the one plan table of a ctx (draw_tab) under draw calls of both kinds.  On one engine, with no synchronisation between them, a
Philox call of 128 segments, a PCG64 call of 128 segments of alternating variants (two launches, side by side in the table) and a Philox
call of 49 segments -- the smallest count that leaves the kernel arguments -- each into its own range of one canary-filled buffer: three
calls in stream order is the smallest shape in which a later call's copy could overwrite a table an earlier launch still reads.  The whole
buffer is compared with NumPy as bytes, and the generators continue NumPy's streams."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEY = bytes(range(32))
CANARY = -7.25
PCG = ["PCG64", "PCG64DXSM"]


def _philox(s, salt):
    g = np.random.Generator(np.random.Philox(key=np.array([s, salt], dtype=np.uint64)))
    g.random(s % 5)
    return g


def _pcg(s):
    g = np.random.Generator(getattr(np.random, PCG[s % 2])(s))
    g.random(s % 4)
    return g


def test_three_calls_of_two_kinds_in_stream_order_share_the_table():
    from flashe_amd import Engine
    eng = Engine(KEY, 64)
    calls = [("philox_random_dev", [_philox(s, 7) for s in range(128)], [_philox(s, 7) for s in range(128)]),
             ("pcg64_random_dev", [_pcg(s) for s in range(128)], [_pcg(s) for s in range(128)]),
             ("philox_random_dev", [_philox(s, 9) for s in range(49)], [_philox(s, 9) for s in range(49)])]
    at, layout = 1, []
    for _call, gens, _refs in calls:
        counts = [1 + (37 * s) % 1500 for s in range(len(gens))]
        offsets = []
        for n in counts:
            offsets.append(at)
            at += n + 1                              # a canary draw between any two ranges
        layout.append((counts, offsets))
    total = at + 5
    want = np.full(total, CANARY)
    buf = eng.upload(np.full(total, CANARY))
    for (call, gens, _refs), (counts, offsets) in zip(calls, layout):
        getattr(eng, call)(gens, counts, out=buf, offsets=offsets)                      # (no sync: the next call follows at once)
    for (_call, _gens, refs), (counts, offsets) in zip(calls, layout):
        for r, n, off in zip(refs, counts, offsets):
            want[off:off + n] = r.random(n)
    got = buf.download(np.float64, total)
    assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want)[:8]
    for _call, gens, refs in calls:
        for s, (g, r) in enumerate(zip(gens, refs)):
            assert g.random(5).tobytes() == r.random(5).tobytes(), s
