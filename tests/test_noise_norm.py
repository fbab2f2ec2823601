"""cn_noise_norm on the CPU: the entry point in the header, the library and the C# binding; the k_noise_norm instantiations' registers and
memory instructions in the gfx950 code object; the model of its composition and reduction (tests/noise_norm_model.py) against Python
integers; the range merging of levels.min_budget."""
import os
import random
import re
import subprocess
import sys
from types import SimpleNamespace

import pytest

from noise_norm_model import centred, norm_words, prod, value, y_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "cryptonets_amd", "lib", "obj")

C3 = [0x7fffffd8001, 0x7fffffc8001, 0xfffffffc001, 0xffffff6c001, 0xfffffebc001]
C9 = [0xfffffffd8001, 0xfffffffa0001, 0xfffffff00001, 0x1fffffff68001, 0x1fffffff50001, 0x1ffffffee8001, 0x1ffffffea0001, 0x1ffffffe88001,
      0x1ffffffe48001]
C12 = C3 + C9[:7]
LARGE = [(1 << 61) - 1, 0x1fffffffffe00001, 0x1fffffffffc80001, 0x1fffffffffb40001]     # coprime moduli just below 2^61: the widest sums allowed


# ------------------------------------------------------------------ the entry point
def test_noise_norm_is_declared_exported_and_bound():
    from cryptonets_amd import _native
    hdr = open(os.path.join(ROOT, "include", "cnhip.h")).read()
    assert re.search(r"\bint cn_noise_norm\(cn_ctx \*ctx, cn_handle ct, uint32_t ci, uint32_t count, uint64_t \*host", hdr)
    assert "cn_noise_norm" in _native.SIGNATURES
    _native.build()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _native.LIB_PATH], text=True)
    assert re.search(r"\bT cn_noise_norm$", syms, flags=re.M)
    cs = open(os.path.join(ROOT, "integration", "CnHip.cs")).read()
    assert re.search(r"public static extern int cn_noise_norm\(IntPtr ctx, ulong ct, uint ci, uint count, \[Out\] ulong\[\] host\);", cs)


# ------------------------------------------------------------------ the kernels in the code object
# k_noise_norm<K>: 512-thread workgroups; at most 96 VGPRs (measured 56, 67 and 79 for K = 5, 9, 12), so a SIMD holds five waves and a CU
# at least two workgroups.  Reloading the constants per limb (nn_launder) keeps the K (K - 1) words of q/q_j out of the SGPRs: hoisted, they
# spilled from K = 4 on.
NN_VGPR_BUDGET = 96


def _resources():
    from cryptonets_amd import _native
    _native.build()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    return kernel_resources, kernel_resources.resources(os.path.join(OBJ, "cn_l_noise.o"))


@pytest.mark.parametrize("k", [5, 9, 12])
def test_noise_norm_kernel_has_no_spills_and_fits_its_budget(k):
    _, res = _resources()
    cand = [name for name in res if name.startswith("void k_noise_norm<%d>" % k)]
    assert cand, "k_noise_norm<%d> not in the gfx950 code object (have %s)" % (k, sorted(res)[:4])
    r = res[cand[0]]
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, r
    assert r["vgpr"] + r["agpr"] <= NN_VGPR_BUDGET, r


def test_every_limb_count_has_a_kernel():
    _, res = _resources()
    for k in range(1, 13):
        assert any(name.startswith("void k_noise_norm<%d>" % k) for name in res), k


def test_noise_norm_kernel_uses_global_not_flat_memory_instructions():
    kr, _ = _resources()
    assert not kr.flat_instructions(os.path.join(OBJ, "cn_l_noise.o"))


# ------------------------------------------------------------------ the model against Python integers
def _edge_values(Q):
    out = [0, 1, Q - 1, (Q - 1) // 2, (Q + 1) // 2, Q // 2]
    for b in range(64, Q.bit_length(), 64):
        out += [(1 << b) - 1, 1 << b, Q - (1 << b), Q - (1 << b) + 1]
    return out


@pytest.mark.parametrize("chain", ["c3", "c9", "c12", "large"])
def test_model_composition_equals_python_integers(chain):
    full = {"c3": C3, "c9": C9, "c12": C12, "large": LARGE}[chain]
    rnd = random.Random(5)
    for k in range(1, len(full) + 1):
        q = full[:k]
        Q = prod(q)
        for X in _edge_values(Q) + [rnd.randrange(Q) for _ in range(40)]:
            assert value(norm_words(y_of(X, q), q)) == centred(X, Q), (chain, k, X)


@pytest.mark.parametrize("chain", ["c3", "c12", "large"])
def test_model_corrects_an_estimate_off_by_one_either_way(chain):
    """the exactness argument of cn_k_noise.hip.h: any estimate alpha - 1, alpha, alpha + 1 of floor(S / q) ends at the same word"""
    full = {"c3": C3, "c12": C12, "large": LARGE}[chain]
    rnd = random.Random(6)
    for k in range(2, len(full) + 1):
        q = full[:k]
        Q = prod(q)
        for X in _edge_values(Q) + [rnd.randrange(Q) for _ in range(10)]:
            y = y_of(X, q)
            alpha = sum(v * (Q // m) for v, m in zip(y, q)) // Q
            for a in (alpha - 1, alpha, alpha + 1):
                if a >= 0:
                    assert value(norm_words(y, q, a)) == centred(X, Q), (chain, k, X, a)


# ------------------------------------------------------------------ levels.min_budget: one probe per contiguous range
class _Client:
    def __init__(self, budgets):
        self.budgets, self.calls = budgets, []

    def noise_budget(self, h, first, count):
        self.calls.append((h, first, count))
        return [self.budgets[(h, first + i)] for i in range(count)]


def test_min_budget_probes_each_contiguous_range_once(monkeypatch):
    from cryptonets_amd import levels
    rnd = random.Random(7)
    clients = [_Client({}), _Client({})]
    env = SimpleNamespace(Environments=[SimpleNamespace(client=c) for c in clients])
    monkeypatch.setattr(levels, "_env_at", lambda e, limbs: env)
    factory = SimpleNamespace(AllocateComputationEnv=lambda: env)
    cols, every = [], []
    # 845 one-ciphertext columns of one handle per prime, a gap, then columns of a second handle
    layout = [(11, i) for i in range(845)] + [(11, 900), (11, 901), (12, 0), (12, 1)]
    for h, i in layout:
        atoms = []
        for p, c in enumerate(clients):
            c.budgets[(h + 100 * p, i)] = b = rnd.randrange(5, 60)
            every.append(b)
            atoms.append(SimpleNamespace(encData=SimpleNamespace(h=h + 100 * p, first=i, count=1)))
        cols.append(SimpleNamespace(eVectors=atoms))
    m = SimpleNamespace(Limbs=None, leVectors=cols)
    assert levels.min_budget([m], factory) == float(min(every))
    for p, c in enumerate(clients):
        assert c.calls == [(11 + 100 * p, 0, 845), (11 + 100 * p, 900, 2), (12 + 100 * p, 0, 2)]
