"""The key-switch planner of cryptonets_amd/csrc/cn_ks_plan.h on the CPU: tests/cpp/ks_plan.cpp builds the tables of every parameter set of the suite
(cn_tables.cpp, plain g++) and prints the plan cn_ks_plan gives over a grid of switches, key forms and ciphertext counts, the answers of the readers beside it
and the refusal of every (form, call shape).  Every line is recomputed here from the moduli with Python integers, from the rules as the code BEFORE the planner
spelt them in six places (ks_planned_mode, ks_pair14_ok, do_keyswitch and its split14 branch, the launchers' pair14 and launch_fused_x, flush_staged_group):
an independent second statement, like test_policy_table.check for the policy.  The anchors are that code's answers for the workloads, as literals.
A second build of the same program runs under -fsanitize=undefined,address: host code in a stand-alone program."""
import itertools
import os
import subprocess
import tempfile

import pytest

from oracle.cno import COEFF_MODULUS_128
from test_policy_table import ALL_SETS, CSRC, ROOT

DIGIT_MAX, WIDE_MAX = 10, 160                               # (ciphertext, limb) blocks: per digit up to 10, two launches up to 160
BIG = 24 << 30
ERR_ARG = -1
DIGITS_MSG = "internal: ready-made digits outside the FP64 register-radix key switch"
PERM_MSG = "internal: automorphism inside the fused key switch"
F64KEY_MSG = "internal: FP64 key without FP64 kernel"


def build(extra=()):
    exe = os.path.join(tempfile.mkdtemp(), "ks_plan")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", *extra, os.path.join(ROOT, "tests", "cpp", "ks_plan.cpp"),
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
    """{set: (header, {plan key: plan}, {reader key: answers}, {refusal key: (rc, text)})}"""
    out = {}
    for line in text.split("\n"):
        w = line.split()
        if not w:
            continue
        if w[0] == "set":
            hdr = dict(zip(("n", "logn", "k", "rl_tot", "gk_tot", "dbc", "gdbc", "f64ok", "arena_small"), map(int, w[2:11])))
            hdr["q"] = [int(x, 16) for x in w[11:]]
            plans, readers, refusals = {}, {}, {}
            out[w[1]] = (hdr, plans, readers, refusals)
        elif w[0] == "p":
            key = tuple(map(int, w[1:11]))
            val = (w[12], w[13]) + tuple(map(int, w[14:20]))
            assert w[11] == ":" and plans.get(key, val) == val, line      # (counts of the grid may coincide: 10 // k = 1 at k = 8)
            plans[key] = val
        elif w[0] == "r":
            key = tuple(map(int, w[1:5]))
            assert w[5] == ":" and key not in readers, line
            rest = " ".join(w[6:]).split("|")
            readers[key] = tuple(tuple(map(int, part.split())) for part in rest)
        else:
            assert w[0] == "x", line
            key = (w[1],) + tuple(map(int, w[2:6]))
            assert w[6] == ":" and key not in refusals, line
            refusals[key] = (int(w[7]), " ".join(w[8:]))
    return out


def counts(k):
    return [DIGIT_MAX // k, DIGIT_MAX // k + 1, WIDE_MAX // k, WIDE_MAX // k + 1, 1, 3, 511, 512, 845, 5488]


def u32(x):
    return x & 0xffffffff


# ---- the rules, restated from the code before the planner
def planned_mode(S, wide, rr, arena_max, cnt, galois):
    """ks_planned_mode: 0 the fused kernel, 1 / 2 two launches (per digit / per source limb)"""
    k, tot = S["k"], S["gk_tot"] if galois else S["rl_tot"]
    if not (rr and (wide > 0 or (wide < 0 and u32(cnt * k) <= WIDE_MAX))):
        return 0
    mode = 2 if wide == 2 or (wide < 0 and u32(cnt * k) > DIGIT_MAX and S["logn"] < 14) else 1
    return 0 if cnt * (k if mode == 2 else tot) * S["ctw2"] * 8 > arena_max else mode


def expected_plan(S, key_f64, galois, wide, split, pair, rr, half, xcd, arena_max, cnt):
    k, tot, bits, qmax = S["k"], S["gk_tot"] if galois else S["rl_tot"], S["bits"], max(S["q"])
    light = bits <= 44
    policy = "U64" if not (key_f64 and S["f64ok"]) else ("F64L" if light else "F64")
    mode = planned_mode(S, wide, rr, arena_max, cnt, galois)
    accmax = (1 if bits >= 50 else 1 << min(10, 50 - bits)) if key_f64 else 0xffffffff          # do_keyswitch
    xcd_cts = cnt & ~7 if xcd == 1 else (0x80000000 if xcd == 2 else 0)
    arena, twl, whole = 0, 0, 0
    pair_ok = bool(pair and split and rr and S["logn"] == 14 and half and key_f64 and mode == 0)      # ks_pair14_ok
    if mode:
        form = "LIMB_MAC" if mode == 2 else "DIGIT_MAC"
        arena = cnt * (k if mode == 2 else tot) * S["ctw2"] * 8
    elif pair_ok:
        form, arena = "PAIR14", cnt * S["ctw2"] * 8
        xcd_cts = cnt & ~7 if xcd == 1 else 0
        if not light and bits <= 49:                        # the launcher's pair14()
            accmax = max(accmax, 1 << (52 - bits))
        dbc = S["gdbc"] if galois else S["dbc"]
        whole = int(tot == k and dbc < 64 and (qmax >> dbc) == 0)
    elif rr and key_f64 and S["logn"] == 14 and half and split:      # the split14 branch of do_keyswitch
        form, arena = "SPLIT14", cnt * S["ctw2"] * 8
    elif rr:
        form = "FUSED"
        twl = int(policy != "U64" and S["logn"] <= 13 and tot >= 12)      # KsFwd<AR, L>::lds and launch_fused_x
    else:
        form = "LEGACY"
    return (form, policy, accmax, xcd_cts, arena, twl, whole, int(arena != 0))


def expected_refusal(S, form, key_f64, galois, xi, shape):
    dig, perm, items, nxt = shape & 1, shape & 2, shape & 4, shape & 8
    rr, mode, pair = form != "LEGACY", form in ("DIGIT_MAC", "LIMB_MAC"), form == "PAIR14"
    if dig and not (rr and key_f64 and S["logn"] <= 13 and not galois and not xi):
        return (ERR_ARG, DIGITS_MSG)
    if (perm or items or nxt) and not mode and not (pair and not items):
        return (ERR_ARG, PERM_MSG)
    if not rr and key_f64:
        return (ERR_ARG, F64KEY_MSG)
    return (0, "-")


def sets(tables):
    """per set: what the rules read, from the moduli of the parameter set itself"""
    out = {}
    for name, p in ALL_SETS.items():
        hdr = tables[name][0]
        n, q = p["n"], list(p["q"] or COEFF_MODULUS_128[p["n"]])
        k = len(q)
        dig = lambda w: sum((m.bit_length() + w - 1) // w for m in q)
        S = dict(n=n, logn=n.bit_length() - 1, k=k, rl_tot=dig(p["dbc"]), gk_tot=dig(p["gdbc"]), dbc=p["dbc"], gdbc=p["gdbc"],
                 f64ok=int(all(m < 2 ** 49 for m in q)), arena_small=8 * 2 * k * n * 8, q=q)
        assert hdr == S, (name, hdr, S)
        S.update(ctw2=2 * k * n, bits=max(q).bit_length())
        out[name] = S
    return out


def check(tables):
    assert sorted(tables) == sorted(ALL_SETS)
    checked = 0
    for name, S in sets(tables).items():
        _, plans, readers, refusals = tables[name]
        cs = counts(S["k"])
        grid = itertools.product(range(S["f64ok"] + 1), (0, 1), (-1, 0, 1, 2), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1, 2), (0, 1), sorted(set(cs)))
        want_keys = set()
        for key in grid:
            key_f64, galois, wide, split, pair, rr, half, xcd, small, cnt = key
            want = expected_plan(S, key_f64, galois, wide, split, pair, rr, half, xcd, S["arena_small"] if small else BIG, cnt)
            assert plans[key] == want, (name, key, plans[key], want)
            want_keys.add(key)
            checked += 1
        assert set(plans) == want_keys, name
        for key in itertools.product((-1, 0, 1, 2), (0, 1), (0, 1), (0, 1)):
            wide, rr, perm, small = key
            arena = S["arena_small"] if small else BIG
            on_load = lambda c: int(bool(perm) and planned_mode(S, wide, rr, arena, c, 1) != 0)      # do_galois / rotate_jobs
            largest = lambda bound: next((c for c in range(bound, 1, -1) if on_load(c)), 0)          # rotate_jobs' piece search
            want = (tuple(on_load(c) for c in cs), (largest(64), largest(3)), tuple(int(c * S["k"] <= WIDE_MAX) for c in cs))      # flush_staged_group
            assert readers[key] == want, (name, key, readers[key], want)
            checked += 1
        assert len(readers) == 32
        for key in itertools.product(("LEGACY", "FUSED", "DIGIT_MAC", "LIMB_MAC", "SPLIT14", "PAIR14"), (0, 1), (0, 1), (0, 1), range(16)):
            assert refusals[key] == expected_refusal(S, *key), (name, key, refusals[key])
            checked += 1
        assert len(refusals) == 6 * 2 * 2 * 2 * 16
    return checked


@pytest.fixture(scope="module")
def tables():
    r = run(build())
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return parse(r.stdout.decode())


def test_every_plan_matches_the_rules_restated(tables):
    assert check(tables) > 1000 * len(ALL_SETS)


def plan(tables, name, cnt, galois=0, key_f64=1, wide=-1, split=1, pair=1, rr=1, half=None, xcd=None):
    """the plan of a context with its defaults: "ks_xcd" 2 up to N = 8192 and 1 at N = 16384, the half-size tables at N = 16384 with every modulus below 2^49"""
    hdr = tables[name][0]
    half = int(hdr["logn"] == 14 and hdr["f64ok"]) if half is None else half
    xcd = (2 if hdr["logn"] <= 13 else 1) if xcd is None else xcd
    return tables[name][1][(key_f64, galois, wide, split, pair, rr, half, xcd, 0, cnt)]


def test_anchors(tables):
    """what the code before the planner did for the workloads, as literals: (form, policy, accmax, xcd_cts, arena bytes, twl, whole, writes the arena)"""
    c3 = tables["c3"][0]
    assert (c3["k"], c3["rl_tot"], c3["gk_tot"], max(c3["q"]).bit_length()) == (5, 25, 15, 44)      # 44 bits: 2^(50 - 44) = 64 terms between recentrings
    ct3 = 2 * 5 * 8192 * 8
    # CryptoNets: the relinearisation of 845 squares is the fused kernel with LDS twiddles, limb-major XCD order; 2 and 3 ciphertexts take the two two-launch forms
    assert plan(tables, "c3", 845) == ("FUSED", "F64L", 64, 0x80000000, 0, 1, 0, 0)
    assert plan(tables, "c3", 2) == ("DIGIT_MAC", "F64L", 64, 0x80000000, 2 * 25 * ct3, 0, 0, 1)
    assert plan(tables, "c3", 3) == ("LIMB_MAC", "F64L", 64, 0x80000000, 3 * 5 * ct3, 0, 0, 1)
    assert plan(tables, "c3", 32)[0] == "LIMB_MAC" and plan(tables, "c3", 33)[0] == "FUSED"
    # LoLa-CIFAR: a rotation of 5488 is pair14 with the whole-limb digit, the k workgroups of a ciphertext on one XCD and the raised accumulator bound
    c5 = tables["c5"][0]
    assert (c5["k"], c5["gk_tot"], max(c5["q"]).bit_length()) == (8, 8, 49)
    ct5 = 2 * 8 * 16384 * 8
    assert plan(tables, "c5", 5488, galois=1) == ("PAIR14", "F64", 8, 5488 & ~7, 5488 * ct5, 0, 1, 1)
    assert plan(tables, "c5", 5488, galois=1)[2] == 8 and plan(tables, "c5", 5488, galois=1, pair=0)[2] == 2      # generic bound at 49 bits: 2
    # N = 16384 has no per-limb form: 20 ciphertexts (160 blocks) are still per digit, 21 are pair14
    assert DIGIT_MAX // 8 + 1 == 2 and plan(tables, "c5", 2, galois=1) == ("DIGIT_MAC", "F64", 2, 0, 2 * 8 * ct5, 0, 0, 1)
    assert plan(tables, "c5", 3, galois=1)[0] == plan(tables, "c5", 3)[0] == "DIGIT_MAC"
    assert plan(tables, "c5", 20, galois=1)[0] == "DIGIT_MAC" and plan(tables, "c5", 21, galois=1)[0] == "PAIR14"
    assert all(p[0] != "LIMB_MAC" for key, p in tables["c5"][1].items() if key[2] == -1)
    assert plan(tables, "c5", 5488, galois=1, pair=0) == ("SPLIT14", "F64", 2, 5488 & ~7, 5488 * ct5, 0, 0, 1)
    assert plan(tables, "c5", 5488, galois=1, split=0) == ("FUSED", "F64", 2, 5488 & ~7, 0, 0, 0, 0)      # the 1024-thread kernel
    assert plan(tables, "c5", 5488, galois=1, split=0, pair=0)[0] == "FUSED"
    # a 60-bit set at N = 16384: the key stays u64 words, fused kernel under the integer policy
    assert plan(tables, "sp-u64-n16384", 845, key_f64=0) == ("FUSED", "U64", 0xffffffff, 845 & ~7, 0, 0, 0, 0)
    assert not tables["sp-u64-n16384"][0]["f64ok"]
    # "legacy_ntt": no register-radix kernels, whatever the rest says
    assert all(p[0] == "LEGACY" for key, p in tables["c3"][1].items() if key[5] == 0)
    assert plan(tables, "c3", 845, key_f64=0, rr=0) == ("LEGACY", "U64", 0xffffffff, 0x80000000, 0, 0, 0, 0)
    # a forced two-launch form whose partial products pass the arena limit falls back: 8 ciphertexts' bytes hold no digit partials of 2 ciphertexts (25 each)
    small = lambda cnt, wide: tables["c3"][1][(1, 0, wide, 1, 1, 1, 0, 2, 1, cnt)][0]
    assert (small(2, 1), small(1, 2), small(2, 2)) == ("FUSED", "LIMB_MAC", "FUSED")


def test_ks_plan_header_is_clean_under_the_sanitizers(tables):
    """-fsanitize=undefined,address with errors fatal over the same sets: the same table, no report"""
    r = run(build(("-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-g")))
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()[-2000:]
    assert parse(r.stdout.decode()) == tables
