"""The plaintext-product planner of cryptonets_amd/csrc/cn_plain_plan.h on the CPU: tests/cpp/plain_plan.cpp builds the tables of every parameter set of the suite
(cn_tables.cpp, plain g++) and prints the plan of every MultiplyPlain over a grid of switches and call shapes, the plans of cn_mul_plain_sum, the SumAllSlots
sequences, the one-launch chains and the row-dot arenas.  Every line is recomputed here from the moduli with Python integers, from the rules as the code BEFORE
the planner spelt them (mul_plain_fused, mul_plain_impl, mul_plain_takes_bcast, sum_slots_chain_elts, cn_rowdot_batch and cn_mul_plain_sum of cn_eval.hip,
cn_rr_ptn_bcast of cn_policy.h, cn_l_mul_plain_sum_kernel / cn_l_mul_ptn_sum_kernel of the launchers): an independent second statement.  The key-switch form a
chain link takes is the restated rule of test_ks_plan.  The anchors are that code's answers for the workloads, as literals.  One difference is on purpose: the old
code refused a chain hand-over on NTT-form rows and in the separate launches and ignored it in lift + product; the plan refuses all three (no caller asks).
A second build of the same program runs under -fsanitize=undefined,address: host code in a stand-alone program."""
import itertools
import os
import subprocess
import tempfile

import pytest

from oracle.cno import COEFF_MODULUS_128
from test_ks_plan import BIG, expected_plan as ks_expected_plan
from test_policy_table import ALL_SETS, CSRC, ROOT

COUNTS = (1, 3, 4, 5, 845, 5488)                          # 4 is the broadcast threshold; 5488: the rows of LoLa-CIFAR
CAP = 1 << 16


def build(extra=()):
    exe = os.path.join(tempfile.mkdtemp(), "plain_plan")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", *extra, os.path.join(ROOT, "tests", "cpp", "plain_plan.cpp"),
                           os.path.join(CSRC, "cn_tables.cpp"), "-o", exe])
    return exe


def run(exe):
    path = os.path.join(tempfile.mkdtemp(), "sets.txt")
    with open(path, "w") as f:
        for name, p in ALL_SETS.items():
            q = p["q"] or []
            f.write("%s %d %d %d %d %d %s\n" % (name, p["n"], p["t"], p["dbc"], p["gdbc"], len(q), " ".join("%x" % x for x in q)))
    return subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


def parse(text):
    """({bits: interval}, {list: (slots, sources, runs)}, {set: {kind: {key: value}}})"""
    intervals, lists, sets, cur = {}, {}, {}, None
    ints = lambda words: tuple(int(x) for x in words)
    for line in text.split("\n"):
        w = line.split()
        if not w:
            continue
        if w[0] == "i":
            intervals[int(w[1])] = int(w[3])
        elif w[0] == "l":
            slot, src, runs = " ".join(w[3:]).split("|")
            lists[w[1]] = (ints(slot.split()), ints(src.split()), tuple(ints(r.split(",")) for r in runs.split()))
        elif w[0] == "set":
            cur = sets[w[1]] = dict(hdr=dict(zip(("n", "logn", "k", "f64ok", "bits"), map(int, w[2:7])), qmax=int(w[7], 16)), m={}, s={}, e={}, c={}, w={})
        else:
            at = w.index(":")
            key, val = ints(w[1:at]), w[at + 1:]
            assert key not in cur[w[0]], line
            if w[0] == "m":
                cur["m"][key] = (val[0], val[1]) + ints(val[2:7]) + (tuple((a.split("=")[0], int(a.split("=")[1])) for a in val[7:]),)
            elif w[0] == "s":
                cur["s"][key] = (int(val[0]), val[1]) + ints(val[2:])
            else:
                cur[w[0]][key] = ints(val)
    return intervals, lists, sets


# ---- the rules, restated from the code before the planner
def policy_of(S, f64):
    return "U64" if not (f64 and S["f64ok"]) else ("F64L" if S["bits"] <= 44 else "F64")


def no_wide_kernel(pol, S):
    return pol == "U64" and S["logn"] == 14                     # cn_rr_ptn_bcast, cn_l_mul_plain_sum_kernel, cn_l_mul_ptn_sum_kernel, diag_has, PtnForm::has


def expected_product(S, f64, fused, bcast, rr, ntt, a_bcast, pstride, alias, chain, polys, count):
    """(form, policy, launches, forward limbs, inverse limbs, ptn_bcast, refused, scratch list)"""
    k, n = S["k"], S["n"]
    pol, npt, item, limbs = policy_of(S, f64), count if pstride else 1, polys * k * n * 8, count * polys * k
    alias = alias and a_bcast
    if not (fused and rr):                                      # mul_plain_impl: the six separate launches
        return ("LEGACY", pol, 1 if ntt else 2, 0, 0, 0, chain, () if ntt else (("lift", npt * k * n * 8),))
    if a_bcast and pstride and count >= 4 and bcast and not (ntt and no_wide_kernel(pol, S)):      # mul_plain_fused, first branch
        return ("BCAST", pol, 1, 0 if ntt else limbs, limbs, ntt, 0, () if chain else (("ctn", item),))
    if ntt:
        return ("PTN_FUSED", pol, 1, limbs, limbs, 0, chain, (("keep", item),) if alias else ())
    # (the old code went on here with a hand-over it could not give: the plan refuses)
    return ("LIFT_FUSED", pol, 2, npt * k + limbs, limbs, 0, chain, (("lift", npt * k * n * 8),) + ((("keep", item),) if alias else ()))


def ptn_interval(qmax):
    bound = qmax // 2 + 1 + -((-3 * qmax * qmax) >> 53)
    fit = (2 ** 52 - 1) // bound
    return min(fit, CAP) if fit else 1


def acc_interval(bits):
    return 1 if bits >= 50 else 1 << min(10, 50 - bits)         # cn_mul_plain_sum and do_keyswitch, the same expression


def expected_sum(S, f64, fused, rr, order, ntt, G, E):
    pol = policy_of(S, f64)
    kernel = int(bool(fused and rr and not no_wide_kernel(pol, S)))
    accmax = 0xffffffff if pol == "U64" else (ptn_interval(S["qmax"]) if ntt else acc_interval(S["bits"]))
    return (kernel, pol, accmax, order, 2 * S["k"] * S["n"] * 8, (G + 1) * 4, E * 4)


def elt_of_step(n, steps):
    return pow(3, steps % (n // 2), 2 * n)


def expected_elts(n, length):
    half, elts = n // 2, []
    ln = length if length else n
    if ln >= half:
        elts.append(2 * n - 1)
        ln = half
    s = 1
    while s < ln:
        elts.append(elt_of_step(n, -s))
        s *= 2
    return tuple(elts)


def ks_form(S, p, key_f64, cnt):
    """the form of a Galois key switch of cnt ciphertexts under a context's defaults (test_ks_plan's restated rule)"""
    q = list(p["q"] or COEFF_MODULUS_128[p["n"]])
    dig = lambda w: sum((m.bit_length() + w - 1) // w for m in q)
    K = dict(n=S["n"], logn=S["logn"], k=S["k"], rl_tot=dig(p["dbc"]), gk_tot=dig(p["gdbc"]), dbc=p["dbc"], gdbc=p["gdbc"], f64ok=S["f64ok"], q=q,
             ctw2=2 * S["k"] * S["n"], bits=S["bits"])
    half = int(S["logn"] == 14 and S["f64ok"])
    return ks_expected_plan(K, key_f64, 1, -1, 1, 1, 1, half, 0, BIG, cnt)[0]


def expected_chain(S, p, ks_chain, keys, cnt, length, loaded=1):
    """sum_slots_chain_elts; loaded: the form of every key (KsKey::f64), but the second link's under keys 1 (missing) and 2 (integer form)"""
    elts = expected_elts(S["n"], length)
    if not (ks_chain and cnt > 0) or len(elts) < 2:
        return ()
    for i, e in enumerate(elts):
        form = (-1 if keys == 1 else 0) if i == 1 and keys else loaded
        if form < 0 or ks_form(S, p, form, cnt) != "PAIR14":
            return ()
    return elts


def check(parsed):
    intervals, lists, sets = parsed
    assert sorted(sets) == sorted(ALL_SETS)
    checked = 0
    for name, T in sets.items():
        p, S = ALL_SETS[name], dict(T["hdr"])
        q = list(p["q"] or COEFF_MODULUS_128[p["n"]])
        assert S == dict(n=p["n"], logn=p["n"].bit_length() - 1, k=len(q), f64ok=int(all(m < 2 ** 49 for m in q)), bits=max(q).bit_length(), qmax=max(q)), name
        grid = list(itertools.product(*[(0, 1)] * 9, (2, 3), COUNTS))
        assert len(T["m"]) == len(grid)
        for key in grid:
            assert T["m"][key] == expected_product(S, *key), (name, key, T["m"][key])
        sums = list(itertools.product(*[(0, 1)] * 5, (1, 2, 100), (1, 3)))
        assert len(T["s"]) == len(sums)
        for f64, fused, rr, order, ntt, G, mult in sums:
            assert T["s"][(f64, fused, rr, order, ntt, G, G * mult)] == expected_sum(S, f64, fused, rr, order, ntt, G, G * mult), (name, f64, fused, rr, ntt, G)
        n = S["n"]
        lengths = (0, 1, 2, 8, n // 2 - 1, n // 2, n)
        for ln in lengths:
            assert T["e"][(ln,)] == expected_elts(n, ln), (name, ln)
        chains = list(itertools.product((0, 1), (0, 1, 2), (0, 2, 21, 5488), sorted(set(lengths))))
        assert len(T["c"]) == len(chains)
        for key in chains:
            assert T["c"][key] == expected_chain(S, p, *key), (name, key, T["c"][key])
        rowdots = list(itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (3, 4, 21, 5488), (1, 8, 0)))
        assert len(T["w"]) == len(rowdots)
        ct = 2 * S["k"] * n * 8
        for f64, bcast, chain, ntt, rows, ln in rowdots:
            # cn_rowdot_batch: length != 1, mul_plain_takes_bcast (here "mp_fused" 1, register-radix), not ptn_fused, and a chain of every key in the form the moduli allow
            takes = bcast and rows >= 4 and not (ntt and no_wide_kernel(policy_of(S, f64), S))
            links = len(expected_chain(S, p, chain, 0, rows, ln, loaded=S["f64ok"])) if ln != 1 and takes else 0
            assert T["w"][(f64, bcast, chain, ntt, rows, ln)] == (links, rows * ct, ct, 0), (name, f64, bcast, chain, ntt, rows, ln)
        checked += len(grid) + len(sums) + len(lengths) + len(chains) + len(rowdots)
    return checked


@pytest.fixture(scope="module")
def parsed():
    r = run(build())
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return parse(r.stdout.decode())


def test_every_plan_matches_the_rules_restated(parsed):
    assert check(parsed) > 5000 * len(ALL_SETS)


def test_the_accumulator_interval_is_both_old_expressions(parsed):
    """bits >= 50 ? 1 : 1 << min(10, 50 - bits), as cn_mul_plain_sum and cn_ks_plan spelt it"""
    assert parsed[0] == {b: acc_interval(b) for b in range(30, 62)}
    assert (parsed[0][30], parsed[0][40], parsed[0][41], parsed[0][49], parsed[0][50], parsed[0][61]) == (1024, 1024, 512, 2, 1, 1)


def test_slots_sources_and_runs(parsed):
    lists = parsed[1]
    assert lists["equal"] == ((0, 0, 0, 0), (7,), ((0, 1),))
    assert lists["increasing"] == ((0, 1, 2, 3, 4), (2, 3, 4, 5, 6), ((0, 5),))
    # 0 1 0 2 3 1 9 5 6 9 4: sources 0 1 2 3 | 9 | 5 6 | 4
    assert lists["interleaved"] == ((0, 1, 0, 2, 3, 1, 4, 5, 6, 4, 7), (0, 1, 2, 3, 9, 5, 6, 4), ((0, 4), (4, 1), (5, 2), (7, 1)))
    assert lists["single"] == ((0,), (11,), ((0, 1),))


def test_anchors(parsed):
    """what the code before the planner did for the workloads, as literals"""
    sets = parsed[2]
    c5 = sets["c5"]
    assert (c5["hdr"]["n"], c5["hdr"]["k"], c5["hdr"]["bits"], c5["hdr"]["f64ok"]) == (16384, 8, 49, 1)
    ct5 = 2 * 8 * 16384 * 8
    # LoLa-CIFAR: the row-dot of 5488 rows is the broadcast product with the one-launch chain behind it, in one arena (ping-pong pair, then the transformed ciphertext)
    key = lambda f64, ntt, chain, cnt=5488: (f64, 1, 1, 1, ntt, 1, 1, 0, chain, 2, cnt)
    assert c5["m"][key(1, 0, 1)] == ("BCAST", "F64", 1, 5488 * 2 * 8, 5488 * 2 * 8, 0, 0, ())
    assert c5["m"][key(1, 0, 0)] == ("BCAST", "F64", 1, 5488 * 2 * 8, 5488 * 2 * 8, 0, 0, (("ctn", ct5),))
    assert c5["w"][(1, 1, 1, 0, 5488, 8)] == (3, 5488 * ct5, ct5, 0) and c5["w"][(1, 1, 1, 1, 5488, 0)] == (14, 5488 * ct5, ct5, 0)
    assert c5["c"][(1, 0, 5488, 8)] == tuple(elt_of_step(16384, -s) for s in (1, 2, 4)) and c5["c"][(1, 0, 5488, 1)] == ()
    assert c5["c"][(1, 0, 5488, 16384)][0] == 2 * 16384 - 1 and len(c5["c"][(1, 0, 5488, 16384)]) == 14
    # ... no chain with "ks_chain" off, with a key missing or in integer form, for 2 ciphertexts (a two-launch key switch), for a single link
    assert c5["c"][(0, 0, 5488, 8)] == c5["c"][(1, 1, 5488, 8)] == c5["c"][(1, 2, 5488, 8)] == c5["c"][(1, 0, 2, 8)] == c5["c"][(1, 0, 5488, 2)] == ()
    assert c5["c"][(1, 0, 21, 8)] != () and c5["w"][(1, 1, 0, 0, 5488, 8)][0] == c5["w"][(1, 0, 1, 0, 5488, 8)][0] == c5["w"][(1, 1, 1, 0, 3, 8)][0] == 0
    # the same under "f64" 0 with NTT-form rows: the product kernel alone, no chain (no wide kernel under the integer policy at N = 16384)
    assert c5["m"][key(0, 1, 0)] == ("PTN_FUSED", "U64", 1, 5488 * 2 * 8, 5488 * 2 * 8, 0, 0, ())
    assert c5["m"][key(0, 1, 1)][6] == 1                         # ... and a hand-over asked of it is refused
    assert c5["w"][(0, 1, 1, 1, 5488, 8)][0] == 0 and c5["w"][(0, 1, 1, 0, 5488, 8)][0] == 3      # (coefficient rows keep the broadcast kernel; the keys are FP64-form)
    assert c5["s"][(0, 1, 1, 0, 1, 100, 300)][:3] == (0, "U64", 0xffffffff) and c5["s"][(1, 1, 1, 0, 0, 100, 300)][:3] == (1, "F64", 2)
    assert c5["s"][(1, 1, 1, 1, 1, 100, 300)][:4] == (1, "F64", ptn_interval(c5["hdr"]["qmax"]), 1)
    # N = 512 has no register-radix kernels (rr_kernels: the `rr` switch is 0): the separate launches, composed sums
    n512 = sets["R512"]
    assert n512["hdr"]["logn"] == 9
    assert all(v[0] == "LEGACY" for key, v in n512["m"].items() if not key[3]) and all(v[0] == 0 for key, v in n512["s"].items() if not key[2])
    assert n512["m"][(1, 1, 1, 0, 0, 0, 1, 0, 0, 2, 3)][2:] == (2, 0, 0, 0, 0, (("lift", 3 * n512["hdr"]["k"] * 512 * 8),))
    # CryptoNets (N = 8192, 44-bit limbs): 3 rows lift + product, 4 rows broadcast; a broadcast source inside the outputs is kept
    c3 = sets["c3"]
    kn3 = 5 * 8192 * 8
    assert c3["m"][(1, 1, 1, 1, 0, 1, 1, 1, 0, 2, 3)] == ("LIFT_FUSED", "F64L", 2, 3 * 5 + 3 * 2 * 5, 3 * 2 * 5, 0, 0, (("lift", 3 * kn3), ("keep", 2 * kn3)))
    assert c3["m"][(1, 1, 1, 1, 1, 1, 1, 1, 0, 2, 4)] == ("BCAST", "F64L", 1, 0, 4 * 2 * 5, 1, 0, (("ctn", 2 * kn3),))
    assert c3["s"][(1, 1, 1, 0, 0, 2, 6)] == (1, "F64L", 64, 0, 2 * kn3, 12, 24)
    assert sets["sp-u64-n16384"]["m"][(1, 1, 1, 1, 1, 1, 1, 0, 0, 2, 4)][0] == "PTN_FUSED" and sets["sp-u64-n8192"]["m"][(1, 1, 1, 1, 1, 1, 1, 0, 0, 2, 4)][0] == "BCAST"


def test_plain_plan_header_is_clean_under_the_sanitizers(parsed):
    """-fsanitize=undefined,address with errors fatal over the same sets: the same table, no report"""
    r = run(build(("-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-g")))
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()[-2000:]
    assert parse(r.stdout.decode()) == parsed
