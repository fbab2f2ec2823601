"""The summed rotations without a GPU: the resources of the BUILT kernels k_ks_term_mac and k_ks_sum_terms (cn_k_ks.hip.h), from the code objects of the three key-switch units like
tests/test_ks_hoist_resources.py - no instantiation spills or touches scratch (at N = 16384 a 1024-thread workgroup leaves 128 registers per thread), the operands
that come out of the device tables stay global accesses, the instantiations are exactly those the planner's predicate admits (cn_ks_sum_built: not the
integer policy at N = 16384; cn_ks_term_built: N <= 8192) - and the C ABI, its Python binding, the generated C# declarations and the header's contract are present."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OBJ = os.path.join(ROOT, "cryptonets_amd", "lib", "obj")
UNITS = {"cn_l_ks_u64.o": "ArU64", "cn_l_ks_f64.o": "ArF64T<1>", "cn_l_ks_f64l.o": "ArF64T<0>"}
SIZES = (10, 11, 12, 13, 14)
NAMES = ("cn_rotate_rows_sum", "cn_apply_galois_sum")


@pytest.fixture(scope="module")
def built():
    from cryptonets_amd import _native
    _native.build()
    import kernel_resources
    return {obj: kernel_resources.resources(os.path.join(OBJ, obj)) for obj in UNITS}


@pytest.mark.parametrize("obj", sorted(UNITS))
def test_every_instantiation_fits_its_workgroup_without_scratch(built, obj):
    res, policy = built[obj], UNITS[obj]
    close = " >" if policy.endswith(">") else ">"
    have = sorted(k for k in res if "k_ks_sum_terms" in k or "k_ks_term_mac" in k)
    want = ["void k_ks_sum_terms<%d, %s%s" % (L, policy, close) for L in SIZES if not (policy == "ArU64" and L == 14)]
    want += ["void k_ks_term_mac<%d, %s%s" % (L, policy, close) for L in SIZES if L <= 13]
    assert have == sorted(want)                              # what the launchers instantiate is what the planner admits
    for name in have:
        r = res[name]
        L = int(name.split("<")[1].split(",")[0])
        budget = 128 if L == 14 else 256                     # 1024 threads: 4 waves per SIMD; up to 512 threads: at least one workgroup per CU at two waves per SIMD
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
        assert r["vgpr"] + r["agpr"] <= budget, (name, r)


def test_table_operands_are_global_accesses(built):
    import kernel_resources
    for obj in UNITS:
        assert not kernel_resources.flat_instructions(os.path.join(OBJ, obj)), obj


def test_abi_binding_and_header_are_present():
    import ctypes
    from cryptonets_amd import _native
    _native.build()
    L = ctypes.CDLL(_native.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name) and name in _native.SIGNATURES
    assert hasattr(_native.Context, "rotate_rows_sum") and hasattr(_native.Context, "apply_galois_sum")
    header = open(os.path.join(ROOT, "include", "cnhip.h")).read()
    assert ("int cn_apply_galois_sum(cn_ctx *ctx, cn_handle in, const uint32_t *ii, const uint64_t *elts, const uint32_t *grp_off, uint32_t G, cn_handle out, "
            "uint32_t oi);") in header
    assert ("int cn_rotate_rows_sum(cn_ctx *ctx, cn_handle in, const uint32_t *ii, const int *steps, const uint32_t *grp_off, uint32_t G, cn_handle out, "
            "uint32_t oi);") in header
    assert '"ks_summed"' in header
    cs = open(os.path.join(ROOT, "integration", "CnHip.cs")).read()
    for name in NAMES:
        assert "public static extern int %s(" % name in cs
