"""cn_mul_plain_sum without a GPU: the resources of the BUILT kernel k_mul_plain_sum (cn_k_diag.hip.h), from the code object like
tests/test_mul_relin_sum_resources.py.  A block keeps the 16 values of a transform and 16 accumulators in registers for all terms of its group: it must not
spill, touch scratch memory or fall to flat memory instructions, and at N = 16384 (1024 threads a workgroup, four waves a SIMD) it has 128 registers a thread.
The integer policy has no instantiation at N = 16384 (it spills there when built: the call composes cn_mul_plain and cn_add_many instead)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OBJ = os.path.join(ROOT, "cryptonets_amd", "lib", "obj", "cn_l_diag.o")

# (log2 N, policy, VGPR budget = what the build reports): 32 registers of transform values, 32 of accumulators (FP64 and 64-bit integers alike), the root and
# ciphertext words in flight.  N <= 8192: workgroups of at most 512 threads, 256 registers a thread available
F64 = ["ArF64T<0>", "ArF64T<1>"]
BUDGETS = ([(10, p, 122) for p in F64] + [(11, p, 121) for p in F64] + [(12, p, 121) for p in F64] + [(13, p, 121) for p in F64] + [(14, p, 116) for p in F64]
           + [(10, "ArU64", 139), (11, "ArU64", 140), (12, "ArU64", 154), (13, "ArU64", 150)])


@pytest.fixture(scope="module")
def built():
    from cryptonets_amd import _native
    _native.build()
    import kernel_resources
    return kernel_resources.resources(OBJ), kernel_resources


def kernel(res, logn, policy):
    hits = [k for k in res if k.replace(" ", "").startswith("voidk_mul_plain_sum<%d,%s>" % (logn, policy.replace(" ", "")))]
    assert len(hits) == 1, "k_mul_plain_sum<%d, %s> not found once (have %s)" % (logn, policy, sorted(res))
    return hits[0], res[hits[0]]


@pytest.mark.parametrize("logn,policy,budget", BUDGETS)
def test_mul_plain_sum_stays_inside_its_budget(built, logn, policy, budget):
    name, r = kernel(built[0], logn, policy)
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
    assert r["lds"] == 0, (name, r)                                  # the exchange image is dynamic LDS, sized at the launch
    assert r["vgpr"] + r["agpr"] <= budget, "%s: %d registers, budget %d" % (name, r["vgpr"] + r["agpr"], budget)
    if logn == 14:
        assert r["vgpr"] + r["agpr"] <= 128, (name, r)


def test_every_instantiation_is_listed_and_the_integer_policy_stops_at_8192(built):
    names = sorted(k.replace(" ", "") for k in built[0] if "k_mul_plain_sum" in k)
    assert names == sorted("voidk_mul_plain_sum<%d,%s>" % (l, p) for (l, p, _) in BUDGETS)


def test_diag_launcher_object_uses_global_not_flat_memory_instructions(built):
    flat = built[1].flat_instructions(OBJ)
    assert not flat, flat
