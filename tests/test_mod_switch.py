"""Modulus switching on the CPU: the rounding model, its consistency with the oracle (slots survive a switch, the key-slicing rule), the
serialization of a level, and the built library (symbols, the kernel in the gfx950 code object and its resources)."""
import io
import os
import random
import re
import sys

import numpy as np
import pytest

from conftest import PARAMS
from modswitch_model import crt_compose, digits, slice_key, slice_poly, switch_bigint, switch_residues

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "cryptonets_amd", "lib", "obj")


def qs(name):
    p = PARAMS[name]
    if p["q"] is not None:
        return list(p["q"])
    from oracle.cno import COEFF_MODULUS_128
    return list(COEFF_MODULUS_128[p["n"]])


# ------------------------------------------------------------------ the rounding model
@pytest.mark.parametrize("name", ["tiny", "c3", "c5"])
def test_residue_formula_equals_bigint_rounding(name):
    q = qs(name)
    k = len(q)
    Q = 1
    for m in q:
        Q *= m
    rnd = random.Random(5)
    xs = [0, 1, Q - 1, Q - 2, Q // 2, Q // 2 + 1] + [rnd.randrange(Q) for _ in range(200)]
    ql = q[-1]
    for j in range(1, 4):                        # x + h crosses a multiple of q_last
        xs += [j * ql - ql // 2 - 1, j * ql - ql // 2, j * ql - ql // 2 + 1]
    n = len(xs)
    words = np.array([[x % m for x in xs] for m in q], dtype=np.uint64).reshape(1, k, n)
    for limbs in range(k - 1, 0, -1):
        got = switch_residues(words, q, n, limbs).reshape(limbs, n)
        for c, x in enumerate(xs):
            exp = switch_bigint(x, q, limbs)
            assert [int(got[i, c]) for i in range(limbs)] == [exp % m for m in q[:limbs]], (limbs, x)
            assert crt_compose([int(got[i, c]) for i in range(limbs)], q[:limbs]) == exp


# ------------------------------------------------------------------ consistency with the oracle
def level_oracle(o, name, limbs, ks_xi=False):
    from oracle.cno import Oracle
    p = PARAMS[name]
    lo = Oracle(p["n"], p["t"], q=o.q[:limbs], dbc=p["dbc"], gdbc=p["gdbc"], ks_xi=ks_xi)
    lo.import_keys(slice_poly(o.secret_key(), o.k, o.n, limbs, 1), slice_poly(o.public_key(), o.k, o.n, limbs, 2))
    return lo


@pytest.mark.parametrize("name,lowest", [("tiny", 1), ("c3", 2)])
def test_switched_ciphertexts_decrypt_unchanged_with_the_sliced_secret_key(name, lowest):
    from oracle.cno import Oracle
    p = PARAMS[name]
    o = Oracle(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"])
    o.keygen(3, galois=False)
    rng = np.random.default_rng(1)
    vals = rng.integers(0, o.t, size=o.n, dtype=np.uint64)
    ct = o.encrypt(o.encode(vals))
    for limbs in range(o.k - 1, lowest - 1, -1):
        lo = level_oracle(o, name, limbs)
        sw = switch_residues(ct, o.q, o.n, limbs)
        assert np.array_equal(lo.decode(lo.decrypt(sw)), vals), limbs


@pytest.mark.parametrize("name,limbs", [("tiny", 2), ("c3", 3)])
def test_sliced_relin_key_relinearizes_at_the_level(name, limbs):
    """ks_xi = 0: the level's keys are exactly the slice of the first level's (entries (l, d) with l < limbs, first limbs limbs)"""
    from oracle.cno import Oracle
    p = PARAMS[name]
    o = Oracle(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"])
    o.keygen(4, galois=False)
    rng = np.random.default_rng(2)
    a = rng.integers(0, 16, size=o.n, dtype=np.uint64)
    b = rng.integers(0, 16, size=o.n, dtype=np.uint64)
    ca, cb = o.encrypt(o.encode(a)), o.encrypt(o.encode(b))
    lo = level_oracle(o, name, limbs)
    lo.import_relin_key(slice_key(o.relin_key(), o.k, o.n, digits(o.q, p["dbc"]), limbs))
    sa, sb = switch_residues(ca, o.q, o.n, limbs), switch_residues(cb, o.q, o.n, limbs)
    prod = lo.relinearize(lo.multiply(sa, sb))
    assert len(prod) == 2 * limbs * o.n
    exp = (a.astype(object) * b.astype(object)) % o.t
    assert [int(v) for v in lo.decode(lo.decrypt(prod))] == [int(v) for v in exp]


# ------------------------------------------------------------------ serialization
def test_level_parms_id_is_the_prefix_parms_id():
    from cryptonets_amd.serialization import Parameters
    p = PARAMS["c3"]
    P = Parameters(p["n"], qs("c3"), p["t"])
    for l in range(1, P.k + 1):
        assert P.level(l).parms_id() == Parameters(p["n"], qs("c3")[:l], p["t"]).parms_id()
    assert len(set(P.chain())) == P.k
    with pytest.raises(ValueError):
        P.level(0)


def test_any_level_loader_accepts_the_chain_and_rejects_foreign_levels():
    from cryptonets_amd.serialization import BadStream, Parameters, load_ciphertext, load_ciphertext_any_level, save_ciphertext
    p = PARAMS["tiny"]
    q = qs("tiny")
    P = Parameters(p["n"], q, p["t"])
    rng = np.random.default_rng(3)
    for l in (3, 2, 1):
        lv = P.level(l)
        for size in (2, 3):
            w = np.stack([rng.integers(0, m, size=p["n"], dtype=np.uint64) for _ in range(size) for m in q[:l]]).reshape(-1)
            buf = io.BytesIO()
            save_ciphertext(buf, w, lv, size=size)
            got, gsize, glimbs = load_ciphertext_any_level(io.BytesIO(buf.getvalue()), P)
            assert (gsize, glimbs) == (size, l) and np.array_equal(got, w)
            if l < 3:                                # the first-level loader keeps refusing a level ciphertext
                with pytest.raises(BadStream):
                    load_ciphertext(io.BytesIO(buf.getvalue()), P)
    # not on the chain: another t, a non-prefix modulus, a residue above its modulus
    for foreign in (Parameters(p["n"], q[:2], p["t"] + 2), Parameters(p["n"], [q[1]], p["t"]), Parameters(p["n"], q[::-1], p["t"])):
        w = np.zeros(2 * foreign.k * p["n"], dtype=np.uint64)
        buf = io.BytesIO()
        save_ciphertext(buf, w, foreign, size=2)
        with pytest.raises(BadStream):
            load_ciphertext_any_level(io.BytesIO(buf.getvalue()), P)
    w = np.zeros(2 * 2 * p["n"], dtype=np.uint64)
    w[p["n"] + 5] = q[1]
    buf = io.BytesIO()
    save_ciphertext(buf, w, P.level(2), size=2)
    with pytest.raises(BadStream):
        load_ciphertext_any_level(io.BytesIO(buf.getvalue()), P)


# ------------------------------------------------------------------ the built library
def test_mod_switch_entry_points_are_declared_and_exported():
    from cryptonets_amd import _native
    hdr = open(os.path.join(ROOT, "include", "cnhip.h")).read()
    for fn in ("cn_ctx_create_level", "cn_mod_switch"):
        assert re.search(r"\bint %s\(" % fn, hdr), fn
        assert fn in _native.SIGNATURES
    _native.build()
    L = _native.lib()
    assert L.cn_ctx_create_level and L.cn_mod_switch


# k_mod_switch<KS, KD>: two coefficients x KS limbs in registers; (KS, KD, VGPR budget): at <= 64 VGPRs a SIMD holds 8 waves - enough to
# keep HBM busy for the C3 / C4 shapes; the 8- and 12-limb forms hold 4-5 and 3 (measured 36, 38, 30, 66, 132 VGPRs)
MS_BUDGETS = [(5, 4, 64), (5, 2, 64), (3, 1, 64), (8, 1, 96), (12, 1, 160)]


@pytest.mark.parametrize("ks,kd,budget", MS_BUDGETS)
def test_mod_switch_kernel_in_code_object_within_budget(ks, kd, budget):
    from cryptonets_amd import _native
    _native.build()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = kernel_resources.resources(os.path.join(OBJ, "cn_l_modswitch.o"))
    name = "void k_mod_switch<%d, %d>(unsigned long const*, unsigned long*, DevConsts const*, unsigned int, unsigned int)" % (ks, kd)
    cand = [kname for kname in res if kname.startswith("void k_mod_switch<%d, %d>" % (ks, kd))]
    assert cand, "k_mod_switch<%d, %d> not in the gfx950 code object (have %s)" % (ks, kd, sorted(res)[:4])
    r = res[cand[0]]
    assert r["vgpr_spill"] == 0 and r["scratch"] == 0, r
    assert r["vgpr"] + r["agpr"] <= budget, (name, r)


def test_mod_switch_kernel_uses_global_not_flat_memory_instructions():
    from cryptonets_amd import _native
    _native.build()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    assert not kernel_resources.flat_instructions(os.path.join(OBJ, "cn_l_modswitch.o"))


# ------------------------------------------------------------------ the wrapper's client side at a level
def test_level_lift_decrypts_to_the_same_plaintext_with_the_first_level_key():
    """hewrapper._level_lift: a ciphertext at q[:l] times Q/Q' is a ciphertext over q with the same plaintext - what a host-side client
    (SEAL at the first level) decrypts and probes level ciphertexts through"""
    from types import SimpleNamespace
    from cryptonets_amd.hewrapper import _level_lift
    from oracle.cno import Oracle
    p = PARAMS["c3"]
    o = Oracle(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"])
    o.keygen(6, galois=False)
    rng = np.random.default_rng(4)
    vals = rng.integers(0, o.t, size=o.n, dtype=np.uint64)
    ct = o.encrypt(o.encode(vals))
    root = SimpleNamespace(k=o.k, n=o.n, q=list(o.q))
    for limbs in (4, 3, 2):
        lv = SimpleNamespace(k=limbs, n=o.n, q=list(o.q[:limbs]))
        lifted = _level_lift(lv, root, switch_residues(ct, o.q, o.n, limbs))
        assert lifted.size == ct.size
        assert np.array_equal(o.decode(o.decrypt(lifted)), vals), limbs


def test_binary_operations_refuse_operands_at_another_level():
    from types import SimpleNamespace
    from cryptonets_amd.hewrapper import AtomicSealBfvEncryptedVector, _check_level
    ctx5, ctx2 = SimpleNamespace(k=5), SimpleNamespace(k=2)
    env5 = SimpleNamespace(ctx=ctx5)
    v5 = AtomicSealBfvEncryptedVector._new(encData=SimpleNamespace(buf=SimpleNamespace(ctx=ctx5)))
    v2 = AtomicSealBfvEncryptedVector._new(encData=SimpleNamespace(buf=SimpleNamespace(ctx=ctx2)))
    _check_level(env5, v5, AtomicSealBfvEncryptedVector._new())
    for args in ((v5, v2), (v2, v5)):
        with pytest.raises(Exception, match="parameter mismatch"):
            _check_level(env5, *args)
    with pytest.raises(Exception, match="parameter mismatch"):
        v5.Add(v2, env5)
