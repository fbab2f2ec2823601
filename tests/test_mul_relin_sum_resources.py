"""cn_mul_relin_sum without a GPU: the resources of the BUILT summing kernel k_product_sum (cn_k_gemm.hip.h), from the code object like
tests/test_packed_resources.py - a streaming kernel that must not spill, touch scratch, use LDS or fall to flat memory instructions; the Python binding;
and the wrapper on the CPU backend, which has no such call and keeps the literal loop."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OBJ = os.path.join(ROOT, "cryptonets_amd", "lib", "obj", "cn_l_gemm.o")

# (digits held per thread, VGPR budget = what the build reports): two sets of twelve 16-byte loads (96 registers), four 64-bit sums of components 0 and 1, 2 ND digit sums
BUDGETS = [(2, 126), (4, 132), (5, 156), (8, 192)]


@pytest.fixture(scope="module")
def built():
    from cryptonets_amd import _native
    _native.build()
    import kernel_resources
    return kernel_resources


@pytest.mark.parametrize("nd,budget", BUDGETS)
def test_product_sum_stays_inside_its_budget(built, nd, budget):
    res = built.resources(OBJ)
    name = "void k_product_sum<%d>" % nd
    assert name in res, "%s not found (have %s)" % (name, sorted(k for k in res if "sum" in k))
    r = res[name]
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
    assert r["lds"] == 0, (name, r)
    assert r["vgpr"] + r["agpr"] <= budget, "%s: %d registers, budget %d" % (name, r["vgpr"] + r["agpr"], budget)


def test_gemm_launcher_object_uses_global_not_flat_memory_instructions(built):
    flat = built.flat_instructions(OBJ)
    assert not flat, flat


def test_binding():
    from cryptonets_amd import _native
    assert "cn_mul_relin_sum" in _native.SIGNATURES
    assert len(_native.SIGNATURES["cn_mul_relin_sum"][1]) == 10
    assert callable(getattr(_native.Context, "mul_relin_sum"))


def test_cpu_backend_keeps_the_literal_loop_and_gives_the_kat_values():
    """BasicOperations.cs:91-109 (MatrixVectorMultiplication) on the CPU backend: no mul_relin_sum there - K mul_relin calls and one add_many per block per prime"""
    from oracle_backend import OracleBackend, make_factory
    from cryptonets_amd.hewrapper import EMatrixFormat, EVectorFormat
    assert not hasattr(OracleBackend, "mul_relin_sum")
    values1 = np.array([-1, 9, 3, 20, 1000, -6945], dtype=float)
    values_m = np.array([[1, -2, 3, -44, 5, 7], [99, 12, -88, 22, 16, 13]], dtype=float)
    f = make_factory("cpu")
    env = f.AllocateComputationEnv()
    calls = {"mul_relin": 0, "add_many": 0}
    for e in env.Environments:
        for name in calls:
            def counted(*a, _f=getattr(e.ctx, name), _n=name, **kw):
                calls[_n] += 1
                return _f(*a, **kw)
            setattr(e.ctx, name, counted)
    mat = f.GetEncryptedMatrix(values_m, EMatrixFormat.ColumnMajor, 12.0)
    sparse = f.GetEncryptedVector(values1, EVectorFormat.sparse, 12.0)
    got = np.asarray(mat.Mul(sparse, env).Decrypt(env), dtype=float)
    assert np.array_equal(got, values_m @ values1)
    primes = len(env.Environments)
    assert calls == {"mul_relin": 6 * primes, "add_many": primes}
