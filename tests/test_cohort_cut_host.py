"""CPU-only: the cut rule of a short cohort's summed chain (flashe_amd/csrc/cohort_cut.h: into how many runs of consecutive clients one
launch cuts it) over a grid of clients, lengths, chip sizes and layouts -- 1 <= parts <= min(16, C), the pieces tile [0, C), C + parts
streams fit the launch's table, one piece from half an item per wave upward, n = 1 and n = 2^32 - 1 -- built with AddressSanitizer + UBSan
(tests/host_cohort_cut_check.cpp); and the Python mirror plan_cohort uses (flashe_amd.block.cohort_cut_parts) against the table the
program prints, row by row."""
import os
import subprocess

from conftest import ROOT


def test_cut_rule_under_sanitizers_and_its_python_mirror(tmp_path):
    from flashe_amd.block import cohort_cut_items, cohort_cut_parts
    exe = tmp_path / "cohort_cut_check"
    src = os.path.join(ROOT, "tests", "host_cohort_cut_check.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "flashe_amd", "csrc"), src, "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1].startswith("COHORT_CUT_OK "), r.stdout[-2000:] + r.stderr[-3000:]
    rows = [tuple(int(v) for v in ln.split()) for ln in lines[:-1]]
    assert len(rows) == int(lines[-1].split()[1]) and len(rows) > 5000
    seen = set()
    for C, n, cus, compact, b, parts in rows:
        assert cohort_cut_parts(C, cohort_cut_items(n, b, 16, bool(compact)), cus) == parts, (C, n, cus, compact, b, parts)
        seen.add(parts)
    assert {1, 2, 4, 8, 10, 16} <= seen and {n for _C, n, *_ in rows} >= {1, 2 ** 32 - 1}
    assert cohort_cut_parts(0, 6, 256) == 0 and cohort_cut_parts(129, 6, 256) == 0 and cohort_cut_parts(3, 0, 256) == 0
