"""cn_diag_scan / cn_diag_encode without a GPU: the resources of the BUILT kernels k_diag_scan and k_diag_gather (cn_k_diagplan.hip.h), from the code object like
tests/test_diag_resources.py.  Both are streaming kernels of a handful of registers: no spill, no scratch memory, no flat memory instruction; the scan keeps its
flags in dynamic LDS (N bytes, sized at the launch), the gather a static tile of 32 x 33 words - the figures DESIGN 6i states."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OBJ = os.path.join(ROOT, "cryptonets_amd", "lib", "obj", "cn_l_diagplan.o")
LDS = {"k_diag_scan": 0, "k_diag_gather": 32 * 33 * 8}              # static bytes (8448 for the tile; the scan's N flag bytes are dynamic)
VGPR = 32                                                            # neither kernel holds more than a few addresses and one or two words


@pytest.fixture(scope="module")
def built():
    from cryptonets_amd import _native
    _native.build()
    import kernel_resources
    return kernel_resources.resources(OBJ), kernel_resources


def test_the_object_holds_exactly_the_two_kernels(built):
    assert sorted(built[0]) == sorted(LDS)


@pytest.mark.parametrize("name", sorted(LDS))
def test_no_spill_no_scratch_and_the_stated_lds(built, name):
    r = built[0][name]
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
    assert r["lds"] <= LDS[name], (name, r)
    assert r["vgpr"] + r["agpr"] <= VGPR, (name, r)


def test_design_states_the_lds_figures():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("## 6i."):text.index("## 7.")]
    assert "8448 bytes" in sec and "N bytes" in sec


def test_launcher_object_uses_global_not_flat_memory_instructions(built):
    flat = built[1].flat_instructions(OBJ)
    assert not flat, flat
