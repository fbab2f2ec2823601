"""Resources of the BUILT reply-path kernels (cn_k_join.hip.h), from the code object like tests/test_packed_resources.py: per-value kernels that keep everything
in registers - no scratch, no spills, no LDS - and reach memory through global, not flat, instructions."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OBJ = os.path.join(ROOT, "cryptonets_amd", "lib", "obj", "cn_l_join.o")

# VGPRs the build reports per instantiation: k_crt_join<P, W> for the shapes of the networks (P = 1, 2, 4, 5) and the largest one, k_join_argmax<W>
PINNED = {
    "void k_crt_join<1, 1>": 16, "void k_crt_join<2, 1>": 26, "void k_crt_join<2, 2>": 26, "void k_crt_join<4, 1>": 30, "void k_crt_join<4, 2>": 30,
    "void k_crt_join<4, 3>": 30, "void k_crt_join<5, 2>": 32, "void k_crt_join<8, 4>": 39,
    "void k_join_argmax<1>": 10, "void k_join_argmax<2>": 14, "void k_join_argmax<3>": 18, "void k_join_argmax<4>": 22,
}


@pytest.fixture(scope="module")
def built():
    from cryptonets_amd import _native
    _native.build()
    import kernel_resources
    return kernel_resources


def test_join_kernels_use_registers_only(built):
    res = built.resources(OBJ)
    joins = {k: r for k, r in res.items() if "k_crt_join" in k or "k_join_argmax" in k}
    assert len([k for k in joins if "k_crt_join" in k]) == 32 and len([k for k in joins if "k_join_argmax" in k]) == 4, sorted(joins)
    for k, r in joins.items():
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0 and r["lds"] == 0 and r["agpr"] == 0, (k, r)
        assert r["vgpr"] <= 64, (k, r)                        # eight waves per SIMD for every instantiation
    for k, vgpr in PINNED.items():
        assert joins[k]["vgpr"] == vgpr, (k, joins[k])


def test_join_kernels_use_global_not_flat_memory_instructions(built):
    flat = built.flat_instructions(OBJ)
    assert not flat, flat
