"""CPU test: the five instantiations of the gapped compact cohort chain (prf_small_cohort_runs_kernel<B>, kernels.hip: the compact cohort
chain over the streams of cipher indices in several runs) fit the budget that keeps one 1,024-thread workgroup resident per CU beside the
AES tables -- no scratch, no VGPR spills, at most 128 VGPRs --, and the kernels whose body they share (prf_small_cohort_kernel<B>,
prf_small_sparse_cohort_kernel<B>) still report the figures of the commit before, per the code objects inside the built library
(tools/kernel_resources.py).  tests/test_cohort_compact_resources.py pins prf_small_chain_kernel<true, unsigned int, B> the same way.  The
entry point that launches the new kernels is declared, exported, bound with its signature and indexed, without an ABI bump."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "flashe_amd", "libflashe_hip.so")
SYM = "flashe_quantize_encrypt_cohort_runs_u32_dev"

WIDTHS = (16, 20, 23, 24, 32)
# vgpr, sgpr_spills as the parent commit's library reported them
PINNED = {
    "prf_small_cohort_kernel": {16: (122, 140), 20: (105, 144), 23: (98, 143), 24: (98, 139), 32: (94, 135)},
    "prf_small_sparse_cohort_kernel": {16: (106, 132), 20: (98, 132), 23: (94, 127), 24: (94, 130), 32: (90, 134)},
}


def _resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    return kernel_resources.resources(LIB)


def test_gapped_compact_cohort_kernels_fit_the_budget():
    res = _resources()
    co = {k: r for k, r in res.items() if "prf_small_cohort_runs_kernel<" in k}
    assert len(co) == 5, sorted(co)
    for b in WIDTHS:
        hit = [r for k, r in co.items() if f"prf_small_cohort_runs_kernel<{b}>(" in k]
        assert len(hit) == 1, (b, sorted(co))
        r = hit[0]
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, (b, r)
        assert r["vgpr"] + r["agpr"] <= 128, (b, r)
        assert r["max_workgroup"] == 1024, (b, r)


@pytest.mark.parametrize("kernel", list(PINNED))
def test_the_kernels_that_share_the_body_keep_their_figures(kernel):
    res = _resources()
    for b, (vgpr, sgpr_spills) in PINNED[kernel].items():
        hit = [r for k, r in res.items() if f"{kernel}<{b}>(" in k]
        assert len(hit) == 1, (b, [k for k in res if kernel in k])
        r = hit[0]
        assert (r["vgpr"], r["sgpr_spills"]) == (vgpr, sgpr_spills), (b, r)
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, (b, r)


def test_the_entry_point_is_declared_exported_bound_and_indexed():
    from flashe_amd import _lib
    assert SYM in _lib.EXPORTED_SYMBOLS and SYM in _lib._SIGNATURES
    lib = _lib.load()
    assert hasattr(lib, SYM)
    # flashe_quantize_encrypt_cohort_u32_dev's arguments with `const uint32_t *idx` in place of first_idx
    res, args = _lib._SIGNATURES[SYM]
    res0, args0 = _lib._SIGNATURES["flashe_quantize_encrypt_cohort_u32_dev"]
    assert res is res0 and len(args) == len(args0) == 14
    assert args[2] is ctypes.POINTER(ctypes.c_uint32) and args0[2] is ctypes.c_uint32 and args[:2] + args[3:] == args0[:2] + args0[3:]
    fn = getattr(lib, SYM)
    assert fn.restype is res and list(fn.argtypes) == list(args)
    header = open(os.path.join(ROOT, "include", "flashe.h")).read()
    index = open(os.path.join(ROOT, "include", "ENTRY_POINTS.md")).read()
    assert f"int {SYM}(flashe_ctx *ctx, uint32_t iter, const uint32_t *idx, int n_clients," in header and f"`{SYM}`" in index
    dyn = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert f" T {SYM}" in dyn
    assert lib.flashe_abi_version() == 4
