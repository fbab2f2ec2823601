"""The products on NTT-form plaintexts without a GPU: the resources of the BUILT kernels k_mul_ptn_sum (cn_k_ptn.hip.h) and k_mul_plain_bcast<.., PTN = true>
(cn_k_rr.hip.h), from the code objects like tests/test_diag_resources.py.

k_mul_ptn_sum keeps two sets of 16 accumulators (both polynomials of a group) and the words of two or three chunks of loads in registers for all terms: it must not spill,
touch scratch memory or fall to flat memory instructions, and at N = 16384 (1024 threads a workgroup) it has 128 registers a thread.  The integer policy has no
instantiation of either kernel at N = 16384 (both spill there when built: cn_mul_plain_sum composes the existing calls, the row-dot batch runs k_mul_plain_fused
alone).  The default instantiations of k_mul_plain_bcast keep the register counts they had before the template parameter existed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OBJ_DIR = os.path.join(ROOT, "cryptonets_amd", "lib", "obj")
OBJ = os.path.join(OBJ_DIR, "cn_l_ptn.o")
RR = {"ArU64": "cn_l_rr_u64.o", "ArF64T<1>": "cn_l_rr_f64.o", "ArF64T<0>": "cn_l_rr_f64l.o"}

F64 = ["ArF64T<0>", "ArF64T<1>"]
# k_mul_ptn_sum<L, policy, NP, WS, D>: (log2 N, policy, polynomials per block, register pairs per chunk, chunks requested ahead, VGPR budget = what the build reports)
SUM = ([(l, p, 2, 4, 1, 128) for l in (10, 11, 12, 13) for p in F64] + [(14, "ArF64T<0>", 2, 1, 2, 126), (14, "ArF64T<1>", 2, 1, 2, 128)]
       + [(10, "ArU64", 2, 2, 1, 163), (11, "ArU64", 2, 2, 1, 166), (12, "ArU64", 2, 2, 1, 166), (13, "ArU64", 2, 2, 1, 168)])
# k_mul_plain_bcast<L, policy, true>
BCAST = ([(10, p, 72) for p in F64] + [(11, p, 72) for p in F64] + [(12, p, 74) for p in F64] + [(13, p, 100) for p in F64] + [(14, p, 108) for p in F64]
         + [(10, "ArU64", 153), (11, "ArU64", 153), (12, "ArU64", 153), (13, "ArU64", 168)])
# k_mul_plain_bcast<L, policy, false>: (VGPRs, spilled VGPRs, scratch bytes) of the instantiation launched before this form existed
BCAST_DEFAULT = ([(10, p, 72, 0, 0) for p in F64] + [(11, p, 70, 0, 0) for p in F64] + [(12, p, 84, 0, 0) for p in F64] + [(13, p, 104, 0, 0) for p in F64]
                 + [(14, p, 114, 0, 0) for p in F64]
                 + [(10, "ArU64", 96, 0, 0), (11, "ArU64", 100, 0, 0), (12, "ArU64", 120, 0, 0), (13, "ArU64", 166, 0, 0), (14, "ArU64", 128, 49, 200)])


@pytest.fixture(scope="module")
def built():
    from cryptonets_amd import _native
    _native.build()
    import kernel_resources
    res = {OBJ: kernel_resources.resources(OBJ)}
    for o in RR.values():
        res[o] = kernel_resources.resources(os.path.join(OBJ_DIR, o))
    return res, kernel_resources


def find(res, text):
    hits = [k for k in res if k.replace(" ", "") == text.replace(" ", "")]
    assert len(hits) == 1, "%s not found once (have %s)" % (text, sorted(res))
    return hits[0], res[hits[0]]


def clean(name, r, budget, logn):
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
    assert r["lds"] == 0, (name, r)                                  # the exchange image is dynamic LDS, sized at the launch
    assert r["vgpr"] + r["agpr"] <= budget, "%s: %d registers, budget %d" % (name, r["vgpr"] + r["agpr"], budget)
    if logn == 14:
        assert r["vgpr"] + r["agpr"] <= 128, (name, r)


@pytest.mark.parametrize("logn,policy,np_,ws,depth,budget", SUM)
def test_mul_ptn_sum_stays_inside_its_budget(built, logn, policy, np_, ws, depth, budget):
    name, r = find(built[0][OBJ], "void k_mul_ptn_sum<%d, %s, %d, %d, %d>" % (logn, policy, np_, ws, depth))
    clean(name, r, budget, logn)


@pytest.mark.parametrize("logn,policy,budget", BCAST)
def test_mul_plain_bcast_on_ntt_rows_stays_inside_its_budget(built, logn, policy, budget):
    name, r = find(built[0][RR[policy]], "void k_mul_plain_bcast<%d, %s, true>" % (logn, policy))
    clean(name, r, budget, logn)


@pytest.mark.parametrize("logn,policy,vgpr,spill,scratch", BCAST_DEFAULT)
def test_default_mul_plain_bcast_keeps_its_registers(built, logn, policy, vgpr, spill, scratch):
    name, r = find(built[0][RR[policy]], "void k_mul_plain_bcast<%d, %s, false>" % (logn, policy))
    assert (r["vgpr"] + r["agpr"], r["vgpr_spill"], r["scratch"]) == (vgpr, spill, scratch), (name, r)


def test_every_instantiation_is_listed(built):
    names = sorted(k.replace(" ", "") for k in built[0][OBJ] if "k_mul_ptn_sum" in k)
    assert names == sorted(("voidk_mul_ptn_sum<%d,%s,%d,%d,%d>" % (l, p, n, w, d)).replace(" ", "") for (l, p, n, w, d, _) in SUM)
    for policy, o in RR.items():
        names = sorted(k.replace(" ", "") for k in built[0][o] if "k_mul_plain_bcast" in k and k.replace(" ", "").endswith(",true>"))
        assert names == sorted(("voidk_mul_plain_bcast<%d,%s,true>" % (l, p)).replace(" ", "") for (l, p, _) in BCAST if p == policy)


def test_ptn_launcher_object_uses_global_not_flat_memory_instructions(built):
    flat = built[1].flat_instructions(OBJ)
    assert not flat, flat
