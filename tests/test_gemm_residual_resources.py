"""The matrix-core GEMM kernels of the clipped + residual weight form without a GPU: registers, spills, scratch and LDS of the BUILT kernels of cn_l_gemm.hip, from the
code object (tools/kernel_resources.py), like tests/test_mul_relin_sum_resources.py.

The <.., GemmResidual> instantiations run more steps of the one-plane body, nothing else: no scratch, no spilled register, and not one vector register more than the
P = 1 kernel of the same form (the two-plane kernels they replace need 188 - 210); the digit GEMM of the form spends its saving on five digits per workgroup.
Every other kernel of the object keeps, figure for figure, what it had before the form existed (BEFORE: vgpr, agpr, sgpr, spilled vgpr, spilled sgpr, LDS bytes,
scratch bytes) - the one-plane kernels included: a plan outside the form launches the code it launched before."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OBJ = os.path.join(ROOT, "cryptonets_amd", "lib", "obj", "cn_l_gemm.o")
FIELDS = ("vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "lds", "scratch")

# new instantiation -> the one-plane kernel whose registers and LDS it may use
RESIDUAL = {
    "k_scalar_gemm_mfma<1, false, GemmResidual>": "k_scalar_gemm_mfma<1, false>",
    "k_scalar_gemm_mfma<1, true, GemmResidual>": "k_scalar_gemm_mfma<1, true>",
    "k_scalar_gemm_mfma<1, false, GemmBskForm, GemmResidual>": "k_scalar_gemm_mfma<1, false, GemmBskForm>",
    "k_scalar_gemm_mfma<1, false, GemmYForm, GemmResidual>": "k_scalar_gemm_mfma<1, false, GemmYForm>",
}
# the digit GEMM of the form takes five digits per workgroup instead of three: 160 accumulator registers, and still two workgroups of 256 threads per CU (256 registers)
RESIDUAL_DIGIT = ("k_digit_gemm_mfma<1, 5, GemmResidual>", "k_digit_gemm_mfma<1, 5, int, GemmResidual>")
BEFORE = {
    "k_digit_gemm<10, 5, int>": (136, 0, 106, 0, 13, 0, 0),
    "k_digit_gemm<10, 5>": (136, 0, 106, 0, 13, 0, 0),
    "k_digit_gemm<2, 5, int>": (68, 0, 88, 0, 0, 0, 0),
    "k_digit_gemm<2, 5>": (68, 0, 88, 0, 0, 0, 0),
    "k_digit_gemm_mfma<1, 3, int>": (146, 0, 66, 0, 0, 18432, 0),
    "k_digit_gemm_mfma<1, 3>": (146, 0, 66, 0, 0, 18432, 0),
    "k_digit_gemm_mfma<2, 3, int>": (206, 0, 68, 0, 0, 18432, 0),
    "k_digit_gemm_mfma<2, 3>": (206, 0, 68, 0, 0, 18432, 0),
    "k_digit_gemm_mfma<3, 2, int>": (208, 0, 64, 0, 0, 12288, 0),
    "k_digit_gemm_mfma<3, 2>": (208, 0, 64, 0, 0, 12288, 0),
    "k_product_sum<2, int>": (126, 0, 58, 0, 0, 0, 0),
    "k_product_sum<2>": (126, 0, 58, 0, 0, 0, 0),
    "k_product_sum<4, int>": (132, 0, 60, 0, 0, 0, 0),
    "k_product_sum<4>": (132, 0, 60, 0, 0, 0, 0),
    "k_product_sum<5, int>": (156, 0, 62, 0, 0, 0, 0),
    "k_product_sum<5>": (156, 0, 62, 0, 0, 0, 0),
    "k_product_sum<8, int>": (192, 0, 64, 0, 0, 0, 0),
    "k_product_sum<8>": (192, 0, 64, 0, 0, 0, 0),
    "k_scalar_gemm<1, false>": (32, 0, 65, 0, 0, 0, 0),
    "k_scalar_gemm<1, true>": (26, 0, 44, 0, 0, 0, 0),
    "k_scalar_gemm<10, false>": (73, 0, 76, 0, 0, 0, 0),
    "k_scalar_gemm<10, true>": (74, 0, 56, 0, 0, 0, 0),
    "k_scalar_gemm<5, false>": (52, 0, 66, 0, 0, 0, 0),
    "k_scalar_gemm<5, true>": (49, 0, 45, 0, 0, 0, 0),
    "k_scalar_gemm_f64<1, 1, 0, false>": (30, 0, 74, 0, 0, 0, 0),
    "k_scalar_gemm_f64<1, 1, 0, true>": (26, 0, 74, 0, 0, 0, 0),
    "k_scalar_gemm_f64<1, 2, 22, false>": (32, 0, 74, 0, 0, 0, 0),
    "k_scalar_gemm_f64<1, 2, 22, true>": (30, 0, 74, 0, 0, 0, 0),
    "k_scalar_gemm_f64<1, 3, 17, false>": (36, 0, 74, 0, 0, 0, 0),
    "k_scalar_gemm_f64<1, 3, 17, true>": (36, 0, 74, 0, 0, 0, 0),
    "k_scalar_gemm_f64<10, 1, 0, false>": (76, 0, 106, 0, 42, 0, 0),
    "k_scalar_gemm_f64<10, 1, 0, true>": (72, 0, 106, 0, 9, 0, 0),
    "k_scalar_gemm_f64<10, 2, 22, false>": (103, 0, 106, 0, 42, 0, 0),
    "k_scalar_gemm_f64<10, 2, 22, true>": (97, 0, 106, 0, 16, 0, 0),
    "k_scalar_gemm_f64<10, 3, 17, false>": (131, 0, 106, 0, 42, 0, 0),
    "k_scalar_gemm_f64<10, 3, 17, true>": (127, 0, 106, 0, 15, 0, 0),
    "k_scalar_gemm_f64<20, 1, 0, false>": (134, 0, 64, 0, 0, 0, 0),
    "k_scalar_gemm_f64<20, 1, 0, true>": (132, 0, 58, 0, 0, 0, 0),
    "k_scalar_gemm_f64<20, 2, 22, false>": (182, 0, 64, 0, 0, 0, 0),
    "k_scalar_gemm_f64<20, 2, 22, true>": (180, 0, 58, 0, 0, 0, 0),
    "k_scalar_gemm_f64<20, 3, 17, false>": (232, 0, 64, 0, 0, 0, 0),
    "k_scalar_gemm_f64<20, 3, 17, true>": (230, 0, 58, 0, 0, 0, 0),
    "k_scalar_gemm_f64<5, 1, 0, false>": (52, 0, 106, 0, 0, 0, 0),
    "k_scalar_gemm_f64<5, 1, 0, true>": (48, 0, 98, 0, 0, 0, 0),
    "k_scalar_gemm_f64<5, 2, 22, false>": (66, 0, 106, 0, 0, 0, 0),
    "k_scalar_gemm_f64<5, 2, 22, true>": (66, 0, 94, 0, 0, 0, 0),
    "k_scalar_gemm_f64<5, 3, 17, false>": (84, 0, 106, 0, 0, 0, 0),
    "k_scalar_gemm_f64<5, 3, 17, true>": (84, 0, 94, 0, 0, 0, 0),
    "k_scalar_gemm_mfma<1, false, GemmBskForm>": (162, 0, 60, 0, 0, 21504, 0),
    "k_scalar_gemm_mfma<1, false, GemmYForm>": (172, 0, 72, 0, 0, 18432, 0),
    "k_scalar_gemm_mfma<1, false>": (148, 0, 66, 0, 0, 18432, 0),
    "k_scalar_gemm_mfma<1, true>": (152, 0, 62, 0, 0, 18432, 0),
    "k_scalar_gemm_mfma<2, false, GemmBskForm>": (210, 0, 62, 0, 0, 21504, 0),
    "k_scalar_gemm_mfma<2, false, GemmYForm>": (208, 0, 74, 0, 0, 18432, 0),
    "k_scalar_gemm_mfma<2, false>": (192, 0, 68, 0, 0, 18432, 0),
    "k_scalar_gemm_mfma<2, true>": (188, 0, 64, 0, 0, 18432, 0),
    "k_scalar_gemm_mfma<3, false>": (226, 0, 68, 0, 0, 18432, 0),
    "k_scalar_gemm_mfma<3, true>": (224, 0, 66, 0, 0, 18432, 0),
}


@pytest.fixture(scope="module")
def res():
    from cryptonets_amd import _native
    _native.build()
    import kernel_resources
    return {k[len("void "):] if k.startswith("void ") else k: v for k, v in kernel_resources.resources(OBJ).items()}


def test_the_object_holds_the_kernels_it_held_and_the_residual_ones(res):
    assert sorted(res) == sorted(list(BEFORE) + list(RESIDUAL) + list(RESIDUAL_DIGIT))


@pytest.mark.parametrize("name", sorted(RESIDUAL))
def test_residual_kernels_neither_spill_nor_outgrow_the_one_plane_kernel(res, name):
    r, base = res[name], res[RESIDUAL[name]]
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
    assert r["vgpr"] + r["agpr"] <= base["vgpr"] + base["agpr"] and r["lds"] == base["lds"], (name, r, base)


@pytest.mark.parametrize("name", RESIDUAL_DIGIT)
def test_residual_digit_kernels_fit_two_workgroups_per_cu_without_spilling(res, name):
    r = res[name]
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
    assert r["vgpr"] + r["agpr"] <= 256 and r["lds"] == 3 * 10 * 64 * 4 * 4, (name, r)


def test_every_other_kernel_has_the_figures_it_had(res):
    now = {k: tuple(res[k][f] for f in FIELDS) for k in BEFORE}
    assert now == BEFORE, {k: (BEFORE[k], now[k]) for k in BEFORE if now[k] != BEFORE[k]}
