"""CPU-only: the piece rule of a short cohort given by ANY strictly ascending cipher indices (cohort_cut_pieces in
flashe_amd/csrc/cohort_cut.h: every gap is a cut) -- one run is exactly cohort_cut_parts / cohort_cut_begin for C = 1 .. 128, the pinned
examples, the invariants over a fixed-seed fuzz (at most 16 pieces, C + pieces streams fit the table, every run boundary is a piece
boundary, a gapped cohort has two pieces at the least), the refusals (17 runs, unsorted, duplicate, 2^32 - 1, 129 clients) -- as a
stand-alone program built with AddressSanitizer + UBSan (tests/host_cohort_cut_pieces_check.cpp); and the Python mirror plan_cohort uses
(flashe_amd.block.cohort_cut_pieces) against every case the program prints."""
import os
import subprocess

from conftest import ROOT


def test_piece_rule_under_sanitizers_and_its_python_mirror(tmp_path):
    from flashe_amd.block import cohort_cut_pieces
    exe = tmp_path / "cohort_cut_pieces_check"
    src = os.path.join(ROOT, "tests", "host_cohort_cut_pieces_check.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "flashe_amd", "csrc"), src, "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1].startswith("COHORT_CUT_PIECES_OK "), r.stdout[-2000:] + r.stderr[-3000:]
    assert len(lines) - 1 == int(lines[-1].split()[1]) and len(lines) > 3000
    seen, gapped, refused = set(), 0, 0
    for ln in lines[:-1]:
        left, right = ln.split("|")
        items, cus, C, *idx = (int(v) for v in left.split())
        parts, *begins = (int(v) for v in right.split())
        assert len(idx) == C and len(begins) == (parts + 1 if parts else 0)
        assert cohort_cut_pieces(idx, items, cus) == begins, ln
        seen.add(parts)
        gapped += any(b != a + 1 for a, b in zip(idx, idx[1:]))
        refused += parts == 0
    assert set(range(0, 17)) <= seen and gapped > 1000 and refused > 5


def test_the_pinned_examples_of_the_mirror():
    from flashe_amd.block import cohort_cut_items, cohort_cut_pieces
    lenet = [i for i in range(100) if i not in (3, 40, 41, 77, 99)]
    assert cohort_cut_pieces([0, 2], 6, 256) == [0, 1, 2]
    assert cohort_cut_pieces([0, 1, 3, 4], 6, 256) == [0, 2, 4]
    assert cohort_cut_pieces(list(range(24)) + list(range(25, 41)), 6, 256) == list(range(0, 41, 4))
    assert cohort_cut_pieces(lenet, cohort_cut_items(61706, 128, 16), 256) == [0, 3, 15, 27, 39, 56, 74, 84, 95]
    assert cohort_cut_pieces(lenet, 3000, 256) == [0, 3, 39, 74, 95]
    assert cohort_cut_pieces(range(0, 32, 2), 6, 256) == list(range(17))
    assert cohort_cut_pieces(range(0, 34, 2), 6, 256) == []
    assert cohort_cut_pieces([3, 2], 6, 256) == [] and cohort_cut_pieces([2, 2], 6, 256) == [] and cohort_cut_pieces([1, 2 ** 32 - 1], 6, 256) == []
    assert cohort_cut_pieces(range(129), 6, 256) == [] and cohort_cut_pieces([], 6, 256) == []
    # the batched count: half tiles of the batched elements
    assert cohort_cut_items(61706, 128, 16, n_elems=12343) == 2 * 49 and cohort_cut_items(61706, 128, 16) == 484
