"""CPU side of the Galois keys for a caller's own steps (cn_keygen_galois): the NTT-domain automorphism the generation kernel rests on, the hop counts a
direct key saves, and the built code object of k_ksk_gen."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


# ---------------------------------------------------------------- NTT-domain automorphism
def brev(v, bits):
    r = 0
    for i in range(bits):
        r |= ((v >> i) & 1) << (bits - 1 - i)
    return r


def gather_index(n, g):
    """slot i of the library's NTT order (minimal primitive root psi, bit-reversed) holds the value at psi^(2 brev(i) + 1); x -> x^g sends it to the slot
    of the point psi^((2 brev(i) + 1) g): sigma_g(s)^[i] = s^[brev(((2 brev(i) + 1) g mod 2N - 1) / 2)] - the table cn_keygen_galois builds"""
    bits = n.bit_length() - 1
    return np.array([brev((((2 * brev(i, bits) + 1) * g) % (2 * n) - 1) // 2, bits) for i in range(n)], dtype=np.int64)


def sigma_coeff(p, g, q):
    """x -> x^g on coefficients mod q: coefficient i goes to (i g) mod N, negated when (i g) div N is odd (k_galois)"""
    n = p.size
    raw = np.arange(n, dtype=np.int64) * int(g)
    out = np.zeros(n, dtype=np.uint64)
    neg = ((raw // n) & 1).astype(bool)
    out[raw % n] = np.where(neg, (np.uint64(q) - p) % np.uint64(q), p)
    return out


def elt_of_step(n, steps):
    """cn_galois_elt_from_step"""
    m = 2 * n
    if steps == 0:
        return m - 1
    s = n // 2 - (-steps) if steps < 0 else steps
    return pow(3, s, m)


T_OF = {1024: 12289, 4096: 40961}
Q_SMALL = 0xffffee001                      # 36 bits, 1 mod 8192
Q_WIDE = 0x3fffffff000001                  # 54 bits, 1 mod 2^24 (SEAL's CoeffModulus128(2048))


@pytest.mark.parametrize("n", [1024, 4096])
def test_ntt_domain_automorphism_is_the_gather(n):
    from oracle.cno import Oracle
    assert Q_SMALL < 1 << 44 and 1 << 49 < Q_WIDE < 1 << 60 and Q_WIDE % (2 * 4096) == 1 and Q_SMALL % (2 * 4096) == 1
    o = Oracle(n, T_OF[n], q=[Q_SMALL, Q_WIDE], dbc=20, gdbc=20)
    rng = np.random.default_rng(n)
    m = 2 * n
    elts = [3, pow(3, -1, m), m - 1, elt_of_step(n, 169)] + ([elt_of_step(n, -1024)] if n // 2 > 1024 else [])
    for j, q in enumerate(o.q):
        s_hat = rng.integers(0, q, size=n, dtype=np.uint64)
        s = o.ntt_inv(j, s_hat)
        assert np.array_equal(o.ntt_fwd(j, s), s_hat)
        for g in elts:
            want = o.ntt_fwd(j, sigma_coeff(s, g, q))
            assert np.array_equal(want, s_hat[gather_index(n, g)]), "N = %d, q = %d, element %d" % (n, q, g)


# ---------------------------------------------------------------- hop counts
def naf_hops(n, steps, have):
    """key switches of RotateRows(steps) with keys for the elements `have`: cn_rotation_plan of cn_rotation.h - one if the step's own key exists, else the sum
    over the terms of its non-adjacent form (a term of N/2 is skipped); None if a term has no key"""
    if steps == 0:
        return 0
    if elt_of_step(n, steps) in have:
        return 1
    sign, v, terms, i = steps < 0, abs(steps), [], 0
    while v:
        zi = 2 - (v & 3) if v & 1 else 0
        v = (v - zi) >> 1
        if zi:
            terms.append((-zi if sign else zi) * (1 << i))
        i += 1
    if len(terms) == 1:
        return None
    total = 0
    for t in terms:
        if abs(t) == n // 2:
            continue
        h = naf_hops(n, t, have)
        if h is None:
            return None
        total += h
    return total


def default_elements(n):
    m = 2 * n
    out, p3, ip3 = {m - 1}, 3, pow(3, -1, m)
    for _ in range(n.bit_length() - 2):
        out |= {p3, ip3}
        p3, ip3 = p3 * p3 % m, ip3 * ip3 % m
    return out


COLUMNS = "columns"


def lola_rotations(name):
    """EVERY rotation of one image and one plaintext prime, with multiplicity, from the layer shapes of networks.py (N = 8192: rows of 4096 slots); a
    column swap is the entry COLUMNS.  Both networks read MNIST through MNIST_CONV with MapCount [5, 1]: 5 maps of 13 x 13 = 169 outputs.
      Vectorize        map i moves 169 i slots to the right: steps -169 i, i = 1 .. 4
      LoLa only:
      Duplicate(8)     PackingShift = 1024: four copies per row (steps -1024 i, i = 1 .. 3), in both rows: one column swap, then the three steps again
      PackedDense      ceil(100 / 8) = 13 packed rows, each SumAllSlots(1024): the steps -1, -2, .. -512
      Interleave       Shift = -1 over the 13 rows: row i moves i slots to the left, asked for as the step -(4096 - i), i = 1 .. 12
      InterleavedDense 10 rows, each SumAllSlots over all N slots: one column swap and the steps -1, -2, .. -2048
      LoLaSmall only:
      Dense            10 rows, each SumAllSlots over all N slots"""
    from cryptonets_amd import networks
    assert networks.MNIST_CONV["InputShape"] == [28, 28] and networks.MNIST_CONV["KernelShape"] == [5, 5] and networks.MNIST_CONV["Stride"] == [2, 2]
    assert networks.FACTORY_PARAMETERS[name]["n"] == 8192
    side, maps, row = (28 + 1 - 5) // 2 + 1, 5, 4096
    all_slots = [COLUMNS] + [-(1 << s) for s in range(row.bit_length() - 1)]
    rot = [-side * side * i for i in range(1, maps)]
    if name == "LoLa":
        shift, copies, hidden = 1024, 8, 100
        per_row = row // shift
        assert copies == 2 * per_row
        rot += [-shift * i for i in range(1, per_row)] + [COLUMNS] + [-shift * i for i in range(1, per_row)]
        packed = -(-hidden // copies)
        rot += packed * [-(1 << s) for s in range(shift.bit_length() - 1)]
        rot += [-(row - i) for i in range(1, packed)]
    rot += 10 * all_slots
    return rot


def lola_step_families(name):
    """the distinct RotateRows steps of lola_rotations: what a recorded evaluation reports (cn_rotation_steps, tests/test_gpu_galois_steps.py)"""
    return sorted({s for s in lola_rotations(name) if s != COLUMNS})


def lola_key_switches(name):
    """(key switches per image and prime with the default key set, with keys for exactly the network's steps): the figures tools/galois_steps_probe.py
    prints and tests/test_gpu_galois_steps.py finds in the Rotation counters"""
    n = 8192
    rot = lola_rotations(name)
    own = {elt_of_step(n, s) for s in rot if s != COLUMNS}
    default = [1 if s == COLUMNS else naf_hops(n, s, default_elements(n)) for s in rot]
    direct = [1 if s == COLUMNS else naf_hops(n, s, own) for s in rot]
    assert None not in default and None not in direct
    return sum(default), sum(direct)


@pytest.mark.parametrize("name,rotations", [("LoLa", 283), ("LoLaSmall", 134)])
def test_direct_keys_take_one_key_switch_per_rotation(name, rotations):
    n = 8192
    rot = lola_rotations(name)
    assert len(rot) == rotations                                            # LoLa: 4 + 7 + 13 x 10 + 12 + 10 x 13; LoLaSmall: 4 + 10 x 13
    default, direct = lola_key_switches(name)
    assert naf_hops(n, -169, default_elements(n)) == 4 and naf_hops(n, -169, {elt_of_step(n, -169)}) == 1        # 169 = 128 + 32 + 8 + 1
    assert direct == len(rot) < default
    assert default - direct == {"LoLa": 20, "LoLaSmall": 11}[name]         # Vectorize 15 -> 4 (both), Interleave 21 -> 12 (LoLa)
    worst = max(naf_hops(n, s, default_elements(n)) for s in rot if s != COLUMNS)
    assert worst == 4                                                       # a cn_rotate_rows_many round pays its longest member: four rounds, one with direct keys
    print("%s: %d rotations per image and prime, %d distinct steps; key switches default set %d, direct keys %d" % (name, len(rot), len(lola_step_families(name)), default, direct))


def test_self_test_rotates_by_steps_of_the_list():
    """SelfTest with a step list compares RotateRows by steps of THAT list (here steps the default key set of the host client serves) and RotateColumns
    when the column-swap key exists: the same word comparison as with the default +-1"""
    from oracle_backend import make_factory
    F = make_factory("cpu", primes=[40961], n=4096, galois=True)
    env = F.AllocateComputationEnv().Environments[0]
    rep = env.SelfTest(True, steps=[0, 2, -4, 2, 8])
    assert rep is not None and rep["ops"][-3:] == ["RotateRows(2)", "RotateRows(-4)", "RotateColumns"]
    assert rep["tried"][-1][2] is None and "RotateRows(1)" not in rep["ops"]
    with pytest.raises(Exception, match="cannot generate Galois keys for a list of steps"):
        env.GenerateEncryptionKeys(True, steps=[2])


# ---------------------------------------------------------------- built code object (as tests/test_seeded_model.py does for k_seeded)
OBJ = os.path.join(ROOT, "cryptonets_amd", "lib", "obj", "cn_l_keygen.o")
KERNELS = [("void k_ksk_gen<%d, %s>" % (L, pol), 128) for L in (10, 11, 12, 13, 14) for pol in ("ArF64T<0> ", "ArF64T<1> ", "ArU64")]


@pytest.fixture(scope="module")
def ksk_resources():
    from cryptonets_amd import _native
    _native.build()
    import kernel_resources
    return kernel_resources.resources(OBJ)


@pytest.mark.parametrize("kernel,budget", KERNELS)
def test_ksk_gen_stays_inside_its_register_budget(ksk_resources, kernel, budget):
    """128 VGPRs and no scratch at every size: two 512-thread workgroups per CU at N = 8192 (as k_encrypt_split), the one 1024-thread workgroup of
    N = 16384 at four waves per SIMD"""
    assert kernel in ksk_resources, "%s not found (have e.g. %s)" % (kernel, sorted(ksk_resources)[:3])
    r = ksk_resources[kernel]
    assert r["vgpr_spill"] == 0 and r["scratch"] == 0, "%s spills: %s" % (kernel, r)
    assert r["vgpr"] + r["agpr"] <= budget, "%s: %d registers, budget %d" % (kernel, r["vgpr"] + r["agpr"], budget)


def test_ksk_gen_uses_global_not_flat_memory_instructions():
    from cryptonets_amd import _native
    _native.build()
    import kernel_resources
    flat = kernel_resources.flat_instructions(OBJ)
    assert not flat, flat


def test_header_binding_and_library_have_the_entry_points():
    import ctypes
    import re
    from cryptonets_amd import _native
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cnhip.h")).read(), flags=re.S)
    _native.build()
    L = ctypes.CDLL(_native.LIB_PATH)
    cs = open(os.path.join(ROOT, "integration", "CnHip.cs")).read()
    for name in ("cn_keygen_galois", "cn_galois_elts", "cn_rotation_steps"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name + " is not declared in include/cnhip.h"
        assert name in _native.SIGNATURES and hasattr(L, name) and name in cs, name
    for meth in ("keygen_galois", "galois_elts", "rotation_steps"):
        assert callable(getattr(_native.Context, meth))
