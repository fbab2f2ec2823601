"""Resources of the BUILT packed-row kernels (cn_k_packed.hip.h), from the code object like tests/test_build_resources.py: streaming kernels that must
not spill, touch scratch or fall to flat memory instructions."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OBJ = os.path.join(ROOT, "cryptonets_amd", "lib", "obj", "cn_l_packed.o")

# (kernel, VGPR budget = what the build reports, LDS bytes at most: the tile, and the word of the workgroup-wide OR): 8 workgroups of 256 threads per CU at either figure
BUDGETS = [("k_unpack_rows", 18, 8192), ("k_pack_rows", 20, 8192)]


@pytest.fixture(scope="module")
def built():
    from cryptonets_amd import _native
    _native.build()
    import kernel_resources
    return kernel_resources


@pytest.mark.parametrize("kernel,budget,lds", BUDGETS)
def test_packed_kernels_stay_inside_their_budget(built, kernel, budget, lds):
    res = built.resources(OBJ)
    assert kernel in res, "%s not found (have %s)" % (kernel, sorted(res))
    r = res[kernel]
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (kernel, r)
    assert r["vgpr"] + r["agpr"] <= budget, "%s: %d registers, budget %d" % (kernel, r["vgpr"] + r["agpr"], budget)
    assert r["lds"] <= lds, (kernel, r)


def test_packed_kernels_use_global_not_flat_memory_instructions(built):
    flat = built.flat_instructions(OBJ)
    assert not flat, flat
