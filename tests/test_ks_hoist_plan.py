"""The planner of the hoisted rotations (cn_ks_hoist_plan, cryptonets_amd/csrc/cn_ks_plan.h) on the CPU: tests/cpp/ks_hoist_plan.cpp builds the tables of the 15
cells of tests/size_policy_sets.py (cn_tables.cpp, plain g++) and prints the plan over key forms, "legacy_ntt" and rotation counts.  Every line is recomputed here
from the moduli with Python integers: policy by the key's form, the recentring interval, tot k N words of arena whatever n is, one workgroup per (digit, limb) and
per (rotation, limb) - per (rotation, limb, component) at N = 16384 -, the closed forms of the transform counters, and the refusals.  The anchors are literals.
A second build of the same program runs under -fsanitize=undefined,address: host code in a stand-alone program."""
import os
import subprocess
import tempfile

import pytest

from size_policy_sets import CELLS, DIGITS, NAME, Q, SETS, WIDTHS
from test_policy_table import CSRC, ROOT

ERR_ARG = -1
COUNTS = (0, 1, 3, 12, 127, 0x20000000)
EMPTY = "hoisted rotations: an empty list"
NO_RR = 'hoisted rotations need the register-radix kernels (1024 <= N <= 16384, "legacy_ntt" off)'
F64KEY = "internal: FP64 key without FP64 kernel"
NO_U64_14 = "hoisted rotations: no kernel under the integer policy at N = 16384 (it does not fit a 1024-thread workgroup's registers)"
TOO_MANY = "hoisted rotations: too many rotations for one launch"
# every cell at both digit widths (the planner reads gk_tot)
ALL = {"%s-w%d" % (NAME(p, n), w): dict(SETS[NAME(p, n)], dbc=w, gdbc=w, policy=p, width=w) for p, n in CELLS for w in WIDTHS}


def build(extra=()):
    exe = os.path.join(tempfile.mkdtemp(), "ks_hoist_plan")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", *extra, os.path.join(ROOT, "tests", "cpp", "ks_hoist_plan.cpp"),
                           os.path.join(CSRC, "cn_tables.cpp"), "-o", exe])
    return exe


def run(exe):
    path = os.path.join(tempfile.mkdtemp(), "sets.txt")
    with open(path, "w") as f:
        for name, p in ALL.items():
            f.write("%s %d %d %d %d %d %s\n" % (name, p["n"], p["t"], p["dbc"], p["gdbc"], len(p["q"]), " ".join("%x" % x for x in p["q"])))
    return subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


def parse(text):
    """({(policy, logn): built}, {set: (header, {(key_f64, rr, n): (rc, policy, accmax, arena, per_component, blocks_ntt, blocks_mac, fwd, inv, text)})})"""
    built, out = {}, {}
    for line in text.split("\n"):
        w = line.split()
        if not w:
            continue
        if w[0] == "b":
            built[(w[1], int(w[2]))] = int(w[4])
        elif w[0] == "set":
            hdr = dict(zip(("n", "logn", "k", "gk_tot", "gdbc", "f64ok"), map(int, w[2:8])))
            hdr["q"] = [int(x, 16) for x in w[8:]]
            plans = {}
            out[w[1]] = (hdr, plans)
        else:
            assert w[0] == "h" and w[4] == ":", line
            key = tuple(map(int, w[1:4]))
            assert key not in plans, line
            head, text_ = line.split(" | ")
            v = head.split()[5:]
            plans[key] = (int(v[0]), v[1]) + tuple(map(int, v[2:])) + (text_,)
    return built, out


def expected(p, hdr, key_f64, rr, n):
    q, k, N = p["q"], len(p["q"]), p["n"]
    tot = DIGITS[p["policy"]][p["width"]]
    bits = max(q).bit_length()
    f64ok = all(m < 2 ** 49 for m in q)
    policy = "U64" if not (key_f64 and f64ok) else ("F64L" if bits <= 44 else "F64")
    accmax = (1 if bits >= 50 else 1 << min(10, 50 - bits)) if key_f64 else 0xffffffff
    pc = int(N == 16384)
    text = None
    if n == 0:
        text = EMPTY
    elif not rr:
        text = NO_RR
    elif key_f64 and not f64ok:
        text = F64KEY
    elif policy == "U64" and N == 16384:
        text = NO_U64_14
    elif n * k * 2 > 0x7fffffff:
        text = TOO_MANY
    if text:
        return (ERR_ARG, policy, accmax, 0, pc, 0, 0, 0, 0, text)
    return (0, policy, accmax, tot * k * N * 8, pc, tot * k, n * k * (2 if pc else 1), tot * k, n * 2 * k, "-")


@pytest.fixture(scope="module")
def tables():
    r = run(build())
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return parse(r.stdout.decode())


def test_every_plan_matches_the_rules_restated(tables):
    built, sets = tables
    assert sorted(sets) == sorted(ALL) and len(ALL) == 30
    checked = 0
    for name, p in ALL.items():
        hdr, plans = sets[name]
        assert (hdr["n"], hdr["k"], hdr["gk_tot"], hdr["gdbc"], hdr["q"]) == (p["n"], 3, DIGITS[p["policy"]][p["width"]], p["width"], list(Q[p["policy"]]))
        assert sorted(plans) == sorted((f, r, n) for f in (0, 1) for r in (0, 1) for n in COUNTS)
        for key, got in plans.items():
            assert got == expected(p, hdr, *key), (name, key, got, expected(p, hdr, *key))
            checked += 1
    assert checked == 30 * 24
    # the predicate the launchers instantiate by: every register-radix size under every policy but the integer one at N = 16384
    assert built == {(pol, logn): int(10 <= logn <= 14 and not (pol == "U64" and logn == 14)) for pol in ("U64", "F64", "F64L") for logn in range(9, 16)}


def test_anchors(tables):
    """(rc, policy, accmax, arena bytes, per component, workgroups of the two launches, forward and inverse limb transforms, refusal) as literals"""
    _, sets = tables
    plan = lambda name, n, key_f64=1, rr=1: sets[name][1][(key_f64, rr, n)]
    # three rotations at N = 1024, one digit per limb: 3 x 3 digit transforms, 3 x 3 workgroups of both components, 72 KiB of arena - for 127 rotations as well
    assert plan("sp-f64l-n1024-w60", 3) == (0, "F64L", 64, 3 * 3 * 1024 * 8, 0, 9, 9, 9, 18, "-")
    assert plan("sp-f64l-n1024-w60", 127) == (0, "F64L", 64, 3 * 3 * 1024 * 8, 0, 9, 381, 9, 762, "-")
    # 15 digits at width 10; 49-bit moduli recentre every other term
    assert plan("sp-f64-n8192-w10", 12) == (0, "F64", 2, 15 * 3 * 8192 * 8, 0, 45, 36, 45, 72, "-")
    # N = 16384: one workgroup per (rotation, limb, component)
    assert plan("sp-f64-n16384-w60", 3) == (0, "F64", 2, 3 * 3 * 16384 * 8, 1, 9, 18, 9, 18, "-")
    assert plan("sp-f64l-n16384-w10", 127)[4:7] == (1, 39, 762)
    # the integer policy: a key kept as 64-bit words (also of a set that could run FP64), every size but N = 16384
    assert plan("sp-u64-n8192-w10", 3, key_f64=0) == (0, "U64", 0xffffffff, 17 * 3 * 8192 * 8, 0, 51, 9, 51, 18, "-")
    assert plan("sp-f64-n4096-w60", 3, key_f64=0)[:3] == (0, "U64", 0xffffffff)
    assert plan("sp-u64-n16384-w60", 3, key_f64=0) == (ERR_ARG, "U64", 0xffffffff, 0, 1, 0, 0, 0, 0, NO_U64_14)
    assert plan("sp-f64-n16384-w60", 3, key_f64=0)[-1] == NO_U64_14
    # refusals: an empty list first, then "legacy_ntt", an FP64 key of moduli without FP64 tables
    assert plan("sp-f64-n1024-w60", 0, rr=0)[-1] == EMPTY and plan("sp-f64-n1024-w60", 3, rr=0)[-1] == NO_RR
    assert plan("sp-u64-n2048-w60", 3)[-1] == F64KEY and plan("sp-f64l-n2048-w60", 0x20000000)[-1] == TOO_MANY


def test_the_wrapper_knows_the_two_refusals_that_mean_no_kernel_here():
    """hewrapper._rotate_hoisted falls back on exactly the planner's "no kernel for this context" refusals, recognised by how their texts begin"""
    from cryptonets_amd._native import HOISTED_UNAVAILABLE
    assert sorted(t for t in (EMPTY, NO_RR, F64KEY, NO_U64_14, TOO_MANY) if any(t.startswith(u) for u in HOISTED_UNAVAILABLE)) == sorted((NO_RR, NO_U64_14))


def test_ks_hoist_plan_is_clean_under_the_sanitizers(tables):
    """-fsanitize=undefined,address with errors fatal over the same sets: the same table, no report"""
    r = run(build(("-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-g")))
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()[-2000:]
    assert parse(r.stdout.decode()) == tables
