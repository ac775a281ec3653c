"""CPU test: the batched wire kernels (wire_wide.hip) fit the budget of tests/test_wire_client_step_resources.py -- at most 128 VGPRs, no
scratch, no VGPR spills, static LDS no larger than prf_small_chain_kernel's; their entry points are exported, bound and indexed, ABI 4."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "flashe_amd", "libflashe_hip.so")
SYMS = ("flashe_quantize_batch_encrypt_pack_model_dev", "flashe_quantize_batch_encrypt_pack_tensors_dev",
        "flashe_unpack_decrypt_unbatch_unquantize_model_dev")


def test_batched_wire_kernels_fit_the_budget():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.resources(LIB)
    wire = {k: r for k, r in res.items() if "prf_wide_pack_kernel<" in k or "prf_wide_unpack_kernel<" in k}
    assert len(wire) == 12, sorted(wire)                     # {single, double} x bs {5, 6, 7, any} out, bs {5, 6, 7, any} back
    chain_lds = max(r["lds_bytes_static"] for k, r in res.items() if "prf_small_chain_kernel<" in k)
    for k, r in wire.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spills"] == 0, (k, r)
        assert r["vgpr"] + r["agpr"] <= 128, (k, r)
        assert r["max_workgroup"] == 1024, (k, r)
        assert r["lds_bytes_static"] <= chain_lds, (k, r, chain_lds)


def test_the_entry_points_are_exported_bound_and_indexed():
    from flashe_amd import _lib
    lib = _lib.load()
    index = open(os.path.join(ROOT, "include", "ENTRY_POINTS.md")).read()
    for sym in SYMS:
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(lib, sym) and f"`{sym}`" in index, sym
    assert lib.flashe_abi_version() == 4
