"""The planner of the summed rotations (cn_ks_sum_plan, cryptonets_amd/csrc/cn_ks_plan.h) on the CPU: tests/cpp/ks_sum_plan.cpp builds the tables of the 15 cells of
tests/size_policy_sets.py at both digit widths (cn_tables.cpp, plain g++) and prints the plan over key forms, "legacy_ntt", three arena limits and counts of rotated
terms on both sides of each threshold.  Every line is recomputed here from the moduli with Python integers: the granularity by (term, limb) blocks - per digit up
to 10 blocks, per source limb up to 160 at N <= 8192, per term above, per digit whatever the count at N = 16384, "compose" under the integer policy at N = 16384 -, the arena bytes (never above the limit: the coarser granularity first, then "compose"), the compose verdicts with their reasons, the workgroups of both launches and the transform counts in closed form, and the
settle interval of k_ks_sum_terms against the exact worst-case sum at the widest modulus of each policy.  The anchors are literals.
A second build of the same program runs under -fsanitize=undefined,address: host code in a stand-alone program."""
import os
import subprocess
import tempfile

import pytest

from size_policy_sets import CELLS, DIGITS, NAME, Q, SETS, WIDTHS
from test_policy_table import CSRC, ROOT

COUNTS = (0, 1, 3, 4, 40, 53, 54, 126)
ARENAS = (24 << 30, 3 << 20, 1 << 20)
DIGIT_MAX, WIDE_MAX = 10, 160
NONE = "no rotated term"
NO_RR = 'no register-radix kernels (N < 1024 or "legacy_ntt")'
F64KEY = "FP64 keys without FP64 kernels"
NO_ROOM = "the partial products would not fit the key-switch arena"
NO_U64_14 = "no kernel under the integer policy at N = 16384"
ALL = {"%s-w%d" % (NAME(p, n), w): dict(SETS[NAME(p, n)], dbc=w, gdbc=w, policy=p, width=w) for p, n in CELLS for w in WIDTHS}


def build(extra=()):
    exe = os.path.join(tempfile.mkdtemp(), "ks_sum_plan")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", *extra, os.path.join(ROOT, "tests", "cpp", "ks_sum_plan.cpp"),
                           os.path.join(CSRC, "cn_tables.cpp"), "-o", exe])
    return exe


def run(exe):
    path = os.path.join(tempfile.mkdtemp(), "sets.txt")
    with open(path, "w") as f:
        for name, p in ALL.items():
            f.write("%s %d %d %d %d %d %s\n" % (name, p["n"], p["t"], p["dbc"], p["gdbc"], len(p["q"]), " ".join("%x" % x for x in p["q"])))
    return subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


def parse(text):
    """({(policy, logn): built}, {set: (header, {(key_f64, rr, arena, rotated): (form, policy, accmax, settle, partials, arena, blocks_mac, blocks_sum, fwd, inv,
    text)}, {key_f64: (settle, milli_q, worst x 2000)})})"""
    built, out = {}, {}
    for line in text.split("\n"):
        w = line.split()
        if not w:
            continue
        if w[0] == "b":
            built[(w[1], int(w[2]))] = (int(w[4]), int(w[5]))
        elif w[0] == "set":
            hdr = dict(zip(("n", "logn", "k", "gk_tot", "gdbc", "f64ok"), map(int, w[2:8])))
            hdr["q"] = [int(x, 16) for x in w[8:]]
            plans, worst = {}, {}
            out[w[1]] = (hdr, plans, worst)
        elif w[0] == "w":
            worst[int(w[1])] = (int(w[3]), int(w[4]), (int(w[5]) << 64) | int(w[6]))
        else:
            assert w[0] == "s" and w[5] == ":", line
            key = tuple(map(int, w[1:5]))
            assert key not in plans, line
            head, text_ = line.split(" | ")
            v = head.split()[6:]
            plans[key] = (v[0], v[1]) + tuple(map(int, v[2:])) + (text_,)
    return built, out


def interval(bits, key_f64):
    return (1 if bits >= 50 else 1 << min(10, 50 - bits)) if key_f64 else 0xffffffff


def expected(p, key_f64, rr, arena, rot):
    q, k, N = p["q"], len(p["q"]), p["n"]
    tot = DIGITS[p["policy"]][p["width"]]
    bits = max(q).bit_length()
    f64ok = all(m < 2 ** 49 for m in q)
    policy = "U64" if not (key_f64 and f64ok) else ("F64L" if bits <= 44 else "F64")
    acc = interval(bits, key_f64)
    outputs = (rot + 1) // 2 if rot else 1
    ct = 2 * k * N * 8
    compose = lambda text: ("compose", policy, acc, acc, 0, 0, 0, 0, 0, 0, text)
    if not rot:
        return compose(NONE)
    if not rr:
        return compose(NO_RR)
    if key_f64 and not f64ok:
        return compose(F64KEY)
    if policy == "U64" and N == 16384:
        return compose(NO_U64_14)
    blocks = rot * k
    if blocks <= DIGIT_MAX or N == 16384:                     # N = 16384: per digit whatever the count (no per-limb and no per-term kernel there)
        form = "digit"
    elif blocks <= WIDE_MAX:
        form = "limb"
    else:
        form = "term"
    fits = lambda partials: rot * partials * ct <= arena
    if form == "digit" and not fits(tot) and N < 16384:
        form = "limb"                                         # the coarser granularity first
    if form == "limb" and not fits(k):
        form = "term"
    partials = {"digit": tot, "limb": k, "term": 1}[form]
    if not fits(partials):
        return compose(NO_ROOM)
    return (form, policy, acc, acc, partials, rot * partials * ct, rot * partials * k, outputs * k * 2, rot * tot * k, outputs * 2 * k, "-")


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
        hdr, plans, _ = sets[name]
        assert (hdr["n"], hdr["k"], hdr["gk_tot"], hdr["gdbc"], hdr["q"]) == (p["n"], 3, DIGITS[p["policy"]][p["width"]], p["width"], list(Q[p["policy"]]))
        assert sorted(plans) == sorted((f, r, a, n) for f in (0, 1) for r in (0, 1) for a in ARENAS for n in COUNTS)
        for key, got in plans.items():
            assert got == expected(p, *key), (name, key, got, expected(p, *key))
            assert got[5] <= key[2], (name, key)               # arena bytes never above arena_max
            checked += 1
    assert checked == 30 * 96
    # the predicates the launchers instantiate by: k_ks_sum_terms at every register-radix size but the integer policy's N = 16384, k_ks_term_mac up to N = 8192
    assert built == {(pol, logn): (int(10 <= logn <= 14 and not (pol == "U64" and logn == 14)), int(10 <= logn <= 13))
                     for pol in ("U64", "F64", "F64L") for logn in range(9, 16)}


def test_the_settle_interval_holds_the_exact_worst_case_sum(tables):
    """a recentred sum (|x| <= q / 2) plus `settle` partials of at most 2.1 q each stays below 2^52 at the widest modulus of every cell with FP64 keys; integer
    keys never settle (canonical sums)"""
    _, sets = tables
    for name, p in ALL.items():
        qmax = max(p["q"])
        _, _, worst = sets[name]
        assert worst[0][0] == 0xffffffff
        settle, milli, w2000 = worst[1]
        assert (settle, milli) == (interval(qmax.bit_length(), 1), 2100)
        assert w2000 == qmax * (1000 + 2 * settle * milli)
        if p["policy"] != "u64":                              # (FP64 keys of the 60-bit moduli are refused before any sum: "FP64 keys without FP64 kernels")
            assert w2000 < 2000 << 52, name
            assert qmax * (1000 + 2 * (2 * settle) * milli) > 2000 << 50      # the interval is not a needless factor of 8 below the limit
    # the widest modulus of each FP64 policy: 49 bits settle every other addition, 44 bits every 64
    assert sets["sp-f64-n1024-w10"][2][1][0] == 2 and sets["sp-f64l-n1024-w10"][2][1][0] == 64


def test_anchors(tables):
    """(form, policy, accmax, settle, partials per term, arena bytes, workgroups of the two launches, forward and inverse limb transforms, why it composes)"""
    _, sets = tables
    plan = lambda name, rot, key_f64=1, rr=1, arena=ARENAS[0]: sets[name][1][(key_f64, rr, arena, rot)]
    ct = lambda n: 2 * 3 * n * 8
    # three rotated terms in two outputs at N = 1024, width 10: a workgroup per (term, digit, limb), 15 partials per term
    assert plan("sp-f64-n1024-w10", 3) == ("digit", "F64", 2, 2, 15, 3 * 15 * ct(1024), 135, 12, 135, 12, "-")
    # four terms are 12 blocks: per source limb; 40 terms (the 49-bit bound test), 53 the last below 160 blocks; 54: one workgroup per (term, limb)
    assert plan("sp-f64-n1024-w10", 4)[:5] == ("limb", "F64", 2, 2, 3)
    assert plan("sp-f64-n1024-w10", 40) == ("limb", "F64", 2, 2, 3, 40 * 3 * ct(1024), 360, 120, 40 * 15 * 3, 120, "-")
    assert plan("sp-f64-n1024-w10", 53)[0] == "limb"
    assert plan("sp-f64-n1024-w10", 54) == ("term", "F64", 2, 2, 1, 54 * ct(1024), 162, 162, 54 * 15 * 3, 162, "-")
    assert plan("sp-u64-n8192-w10", 126, key_f64=0)[:6] == ("term", "U64", 0xffffffff, 0xffffffff, 1, 126 * ct(8192))
    # N = 16384: per digit whatever the count
    assert plan("sp-f64-n16384-w10", 40) == ("digit", "F64", 2, 2, 15, 40 * 15 * ct(16384), 1800, 120, 1800, 120, "-")
    assert plan("sp-f64l-n16384-w60", 126) == ("digit", "F64L", 64, 64, 3, 126 * 3 * ct(16384), 126 * 9, 63 * 6, 126 * 9, 63 * 6, "-")
    # integer keys (also of a set that could run FP64): every size but N = 16384, no recentring
    assert plan("sp-u64-n8192-w60", 3, key_f64=0) == ("digit", "U64", 0xffffffff, 0xffffffff, 3, 9 * ct(8192), 27, 12, 27, 12, "-")
    assert plan("sp-u64-n16384-w60", 3, key_f64=0)[-1] == NO_U64_14 and plan("sp-f64-n16384-w60", 3, key_f64=0)[-1] == NO_U64_14
    # the arena limit: the coarser granularity first, then "compose"
    assert plan("sp-u64-n2048-w10", 3, key_f64=0, arena=ARENAS[1])[:6] == ("limb", "U64", 0xffffffff, 0xffffffff, 3, 9 * ct(2048))
    assert plan("sp-f64-n1024-w10", 40, arena=ARENAS[1])[:6] == ("term", "F64", 2, 2, 1, 40 * ct(1024))
    assert plan("sp-f64-n1024-w10", 40, arena=ARENAS[2])[-1] == NO_ROOM and plan("sp-f64-n16384-w60", 3, arena=ARENAS[1])[-1] == NO_ROOM
    # compose: nothing rotated, "legacy_ntt", FP64 keys of moduli without FP64 tables
    assert plan("sp-f64-n1024-w60", 0)[-1] == NONE and plan("sp-f64-n1024-w60", 3, rr=0)[-1] == NO_RR and plan("sp-u64-n2048-w60", 3)[-1] == F64KEY


def test_ks_sum_plan_is_clean_under_the_sanitizers(tables):
    """-fsanitize=undefined,address with errors fatal over the same sets: the same table, no report"""
    r = run(build(("-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-g")))
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()[-2000:]
    assert parse(r.stdout.decode()) == tables
