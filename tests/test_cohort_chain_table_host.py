"""CPU-only: the chain tables of the cohort launches (flashe_amd/csrc/cohort_chain_table.h: the link filler, the one uncut summed chain
from a cohort's streams, the pieces of a cut cohort) over stand-ins for ChainTable and SmallChainTable pre-filled with a sentinel, against
closed forms for every non-empty subset of ten clients at first_idx 0 and 2^32 - 12, the edges of one table (128 clients in one run and
in 16, 129 and 144 streams), cohort_cut_parts' pieces at 1 .. 128 clients, and the begins cohort_cut_table declines, built with
AddressSanitizer + UBSan (tests/host_cohort_chain_table_check.cpp)."""
import os
import subprocess

from conftest import ROOT


def test_cohort_chain_tables_against_closed_forms_under_sanitizers(tmp_path):
    exe = tmp_path / "cohort_chain_table_check"
    src = os.path.join(ROOT, "tests", "host_cohort_chain_table_check.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "flashe_amd", "csrc"), src, "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    # 2046 subsets and 4 edge shapes x 3 table / element forms; (2046 subsets + 2 edge shapes) x 2 item counts and 6 x 2 x 2 rule shapes x 2 tables
    assert r.returncode == 0 and "COHORT_CHAIN_TABLE_OK 6150 whole chains, 8240 cut tables" in r.stdout, r.stdout + r.stderr[-3000:]
