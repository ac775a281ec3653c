"""CPU test: the lists kernels of the wire way back fit a 1024-thread workgroup (at most 128 VGPRs, no scratch, no VGPR spills, the
prefix table inside gfx950's 160 KiB of LDS); their entry points are exported, bound and indexed, ABI 4."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lists_kernels_fit_the_budget():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.resources(os.path.join(ROOT, "flashe_amd", "libflashe_hip.so"))
    lists = {k: r for k, r in res.items() if "prf_small_unpack_lists_kernel(" in k or "prf_wide_unpack_lists_kernel<" in k}
    assert len(lists) == 5, sorted(lists)                    # the small kernel; bs {5, 6, 7, any}
    for k, r in lists.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0 and r["vgpr"] + r["agpr"] <= 128, (k, r)
        assert r["max_workgroup"] == 1024 and r["lds_bytes_static"] <= 163840, (k, r)


def test_the_entry_points_are_exported_bound_and_indexed():
    from flashe_amd import _lib
    from flashe_amd.engine import Engine
    lib = _lib.load()
    index = open(os.path.join(ROOT, "include", "ENTRY_POINTS.md")).read()
    for sym in ("flashe_unpack_decrypt_lists_unquantize_model_dev", "flashe_unpack_decrypt_lists_unbatch_unquantize_model_dev"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym) and f"`{sym}`" in index and hasattr(Engine, sym[len("flashe_"):]), sym
    assert lib.flashe_abi_version() == 4
