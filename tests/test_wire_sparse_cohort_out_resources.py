"""CPU: prf_small_pack_cohort_kernel fits a 1024-thread workgroup (no scratch, no VGPR spills, static LDS inside 160 KiB); its entry point
is exported, bound, indexed and on Engine, ABI 4."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "flashe_quantize_encrypt_pack_sparse_cohort_dev"


def test_the_packed_sparse_cohort_kernel_fits_the_budget():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.resources(os.path.join(ROOT, "flashe_amd", "libflashe_hip.so"))
    (k, r), = [(k, r) for k, r in res.items() if "prf_small_pack_cohort_kernel(" in k]
    assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0 and r["max_workgroup"] == 1024 and r["lds_bytes_static"] <= 163840, (k, r)


def test_the_entry_point_is_exported_bound_and_indexed():
    from flashe_amd import _lib
    from flashe_amd.engine import Engine
    lib, index = _lib.load(), open(os.path.join(ROOT, "include", "ENTRY_POINTS.md")).read()
    assert SYM in _lib.EXPORTED_SYMBOLS and hasattr(lib, SYM) and f"`{SYM}`" in index and hasattr(Engine, SYM[len("flashe_"):])
    assert lib.flashe_abi_version() == 4
