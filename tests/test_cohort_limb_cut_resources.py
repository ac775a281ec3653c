"""CPU test: the two instantiations of the cut one-limb cohort chain (prf_limb_cohort_cut_kernel<M>, kernels.hip: int_bits 43 .. 64, M = 2,
and 33 .. 42, M = 3) fit the budget that keeps one 1,024-thread workgroup resident per CU beside the AES tables -- no scratch, at most 128
VGPRs -- per the code objects inside the built library (tools/kernel_resources.py), and the two entry points are exported and bound."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "flashe_amd", "libflashe_hip.so")


def test_cut_one_limb_cohort_kernels_fit_the_budget():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.resources(LIB)
    for m in (2, 3):
        hit = [r for k, r in res.items() if f"prf_limb_cohort_cut_kernel<{m}>(" in k]
        assert len(hit) == 1, (m, [k for k in res if "prf_limb_cohort" in k])
        r = hit[0]
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, (m, r)
        assert r["vgpr"] + r["agpr"] <= 128 and r["max_workgroup"] == 1024, (m, r)


def test_the_entry_points_are_exported_and_bound():
    from flashe_amd import _lib
    from flashe_amd.engine import Engine
    lib = _lib.load()
    for sym in ("flashe_cohort_cut_pieces_u64", "flashe_quantize_encrypt_cohort_cut_u64_dev"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym) and callable(getattr(Engine, sym[len("flashe_"):]))
    assert "flashe_quantize_encrypt_cohort_cut_u64_dev" in _lib.COHORT_LAUNCHES and lib.flashe_abi_version() == 4
