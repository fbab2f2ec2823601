"""Resources of the BUILT request-path kernel (cn_k_split.hip.h), from the code object like tests/test_join_resources.py: k_crt_split<P> for every number of
plaintext primes - no scratch, no spills, eight waves per SIMD, and exactly the LDS of the one tile an image-major input is turned through."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OBJ = os.path.join(ROOT, "cryptonets_amd", "lib", "obj", "cn_l_split.o")

TILE_BYTES = 64 * (16 + 1) * 8                 # CSP_TS slots x (CSP_TC plaintexts + 1 of padding) x 8 bytes
# VGPRs the build reports per instantiation
PINNED = {"void k_crt_split<%d>" % P: (17 if P == 1 else 20) for P in range(1, 9)}


@pytest.fixture(scope="module")
def built():
    from cryptonets_amd import _native
    _native.build()
    import kernel_resources
    return kernel_resources


def test_split_kernels_fit_eight_waves_and_one_tile(built):
    res = built.resources(OBJ)
    splits = {k: r for k, r in res.items() if "k_crt_split" in k}
    assert sorted(splits) == sorted(PINNED), sorted(splits)
    for k, r in splits.items():
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0 and r["agpr"] == 0, (k, r)
        assert r["vgpr"] <= 64, (k, r)
        assert r["lds"] == TILE_BYTES, (k, r)
        assert r["vgpr"] == PINNED[k], (k, r)


def test_split_kernels_use_global_not_flat_memory_instructions(built):
    flat = built.flat_instructions(OBJ)
    assert not flat, flat
