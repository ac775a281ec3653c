"""CPU test: the two instantiations of the gapped one-limb cohort chain (prf_limb_cohort_runs_kernel<M>, kernels.hip: the one-limb cohort
chain over the streams of cipher indices in several runs, int_bits 43 .. 64, M = 2, and 33 .. 42, M = 3) fit the budget that keeps one
1,024-thread workgroup resident per CU beside the AES tables -- no scratch, no VGPR spills, at most 128 VGPRs -- per the code objects inside
the built library (tools/kernel_resources.py), and the kernels whose body they share (prf_limb_cohort_kernel<M>) still report the figures of
the commit before.  The entry point that launches the new kernels is declared, exported, bound with its signature and indexed, without an
ABI bump."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "flashe_amd", "libflashe_hip.so")
SYM = "flashe_quantize_encrypt_cohort_runs_u64_dev"

# vgpr, sgpr, sgpr_spills as the parent commit's library reported them
PINNED = {2: (90, 106, 91), 3: (98, 106, 92)}


def _resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    return kernel_resources.resources(LIB)


def test_gapped_one_limb_cohort_kernels_fit_the_budget():
    res = _resources()
    co = {k: r for k, r in res.items() if "prf_limb_cohort_runs_kernel<" in k}
    assert len(co) == 2, sorted(co)
    for m in (2, 3):
        hit = [r for k, r in co.items() if f"prf_limb_cohort_runs_kernel<{m}>(" in k]
        assert len(hit) == 1, (m, sorted(co))
        r = hit[0]
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, (m, r)
        assert r["vgpr"] + r["agpr"] <= 128, (m, r)
        assert r["max_workgroup"] == 1024, (m, r)
    # a name of its own: the counts other tests take of the chained kernels do not see it
    assert not any("prf_limb_cohort_kernel<" in k or "prf_small_cohort" in k for k in co)


def test_the_kernels_that_share_the_body_keep_their_figures():
    res = _resources()
    for m, (vgpr, sgpr, sgpr_spills) in PINNED.items():
        hit = [r for k, r in res.items() if f"prf_limb_cohort_kernel<{m}>(" in k]
        assert len(hit) == 1, (m, [k for k in res if "prf_limb_cohort" in k])
        r = hit[0]
        assert (r["vgpr"], r["sgpr"], r["sgpr_spills"]) == (vgpr, sgpr, sgpr_spills), (m, r)
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, (m, r)


def test_the_entry_point_is_declared_exported_bound_and_indexed():
    from flashe_amd import _lib
    assert SYM in _lib.EXPORTED_SYMBOLS and SYM in _lib._SIGNATURES and SYM in _lib.COHORT_LAUNCHES
    lib = _lib.load()
    assert hasattr(lib, SYM)
    # flashe_quantize_encrypt_cohort_runs_u32_dev's signature (the vectors' element type does not show in the ctypes signature): the one-run
    # form's arguments with `const uint32_t *idx` in place of first_idx, no decrypt mask
    res, args = _lib._SIGNATURES[SYM]
    res0, args0 = _lib._SIGNATURES["flashe_quantize_encrypt_cohort_runs_u32_dev"]
    assert res is res0 and len(args) == 14 and list(args) == list(args0)
    one = _lib._SIGNATURES["flashe_quantize_encrypt_cohort_u64_dev"][1]
    assert args[2] is ctypes.POINTER(ctypes.c_uint32) and one[2] is ctypes.c_uint32 and args[:2] + args[3:] == one[:2] + one[3:]
    fn = getattr(lib, SYM)
    assert fn.restype is res and list(fn.argtypes) == list(args)
    header = open(os.path.join(ROOT, "include", "flashe.h")).read()
    index = open(os.path.join(ROOT, "include", "ENTRY_POINTS.md")).read()
    assert f"int {SYM}(flashe_ctx *ctx, uint32_t iter, const uint32_t *idx, int n_clients, uint64_t n, uint32_t n_jobs," in header
    assert "int element_bits, const double *u_dev, uint64_t *const *ct_dev, uint64_t *sum_out_dev);" in header
    assert "jzf_flashe.py:349-367" in header[header.index("The one-limb cohort for a round in which clients DROPPED OUT"):header.index(f"int {SYM}(")]
    assert f"`{SYM}`" in index
    dyn = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert f" T {SYM}" in dyn
    assert lib.flashe_abi_version() == 4
    from flashe_amd.engine import Engine
    assert callable(getattr(Engine, "quantize_encrypt_cohort_runs_u64_dev"))
