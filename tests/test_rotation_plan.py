"""The hop planner of cryptonets_amd/csrc/cn_rotation.h on the CPU: tests/cpp/rotation_plan.cpp prints, for five ring sizes and four key sets, the plan or the
refusal of RotateRows(steps) for every step count in [-N/2 - 1, N/2 + 1].  Every line is recomputed here: the elements with elt_of_step, the order of the hops
with the non-adjacent form of tests/bigint_model.py, their number with naf_hops (tests/test_galois_steps_model.py); the literals below spell out a few plans.
Queue-time checks, cn_rotate_rows_many and the executing loop read this one plan, and a wrong hop order gives valid ciphertexts of another rotation.
A second build of the same program runs under -fsanitize=undefined,address: host code in a stand-alone program."""
import os
import subprocess
import tempfile

import pytest

from bigint_model import naf
from test_galois_steps_model import default_elements, elt_of_step, naf_hops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1024, 2048, 4096, 8192, 16384)
DIRECT = (169, -169, 5, -7)
TOO_LARGE, NO_KEY = (-1, "step count too large"), (-3, "Galois key not present")


def key_sets(n):
    return {"default": default_elements(n), "empty": set(), "columns": {2 * n - 1},
            "direct": default_elements(n) | {elt_of_step(n, s) for s in DIRECT}}


def build(extra=()):
    exe = os.path.join(tempfile.mkdtemp(), "rotation_plan")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", *extra, os.path.join(ROOT, "tests", "cpp", "rotation_plan.cpp"), "-o", exe])
    return exe


def run(exe):
    path = os.path.join(tempfile.mkdtemp(), "keys.txt")
    with open(path, "w") as f:
        for n in SIZES:
            for name, have in key_sets(n).items():
                f.write("%s %d %d %s\n" % (name, n, len(have), " ".join(str(e) for e in sorted(have))))
    return subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


def parse(text):
    """{(set, n): {steps: (own element, refusal (code, text) or None, [elements])}}"""
    out, rows = {}, None
    for line in text.split("\n"):
        w = line.split()
        if not w:
            continue
        if w[0] == "set":
            rows = out[(w[1], int(w[2]))] = {}
            continue
        assert w[0] == "s" and rows is not None and int(w[1]) not in rows, line
        if w[3] == "refused":
            rows[int(w[1])] = (int(w[2]), (int(w[4]), " ".join(w[5:])), [])
        else:
            assert w[3] == "plan", line
            rows[int(w[1])] = (int(w[2]), None, [int(x) for x in w[4:]])
    return out


def expected(n, steps, have):
    """(refusal or None, elements): the direct key wins, else the terms of the non-adjacent form from low order first, N/2 skipped"""
    if steps == 0:
        return None, []
    if abs(steps) >= n // 2:
        return TOO_LARGE, []
    if elt_of_step(n, steps) in have:
        return None, [elt_of_step(n, steps)]
    terms = naf(steps)
    elts = [elt_of_step(n, t) for t in terms if abs(t) != n // 2]
    if len(terms) == 1 or any(e not in have for e in elts):
        return NO_KEY, []
    return None, elts


@pytest.fixture(scope="module")
def plans():
    r = run(build())
    assert r.returncode == 0, r
    return parse(r.stdout.decode())


def test_every_plan_matches_the_model(plans):
    assert sorted(plans) == sorted((name, n) for n in SIZES for name in key_sets(n))
    checked = 0
    for n in SIZES:
        for name, have in key_sets(n).items():
            rows = plans[(name, n)]
            assert sorted(rows) == list(range(-n // 2 - 1, n // 2 + 2)), (name, n)
            for steps, (own, refusal, elts) in rows.items():
                assert own == (0 if abs(steps) >= n // 2 else elt_of_step(n, steps)), (name, n, steps)
                assert (refusal, elts) == expected(n, steps, have), (name, n, steps)
                hops = naf_hops(n, steps, have) if abs(steps) < n // 2 else None
                assert hops == (None if refusal else len(elts)), (name, n, steps)
                checked += 1
    assert checked == 4 * sum(n + 3 for n in SIZES)


def test_anchors(plans):
    for n in SIZES:
        e = lambda s: elt_of_step(n, s)
        d, own = plans[("default", n)], plans[("direct", n)]
        assert d[-7][1:] == (None, [e(1), e(-8)]) and d[5][1:] == (None, [e(1), e(4)]) and d[3][1:] == (None, [e(-1), e(4)])
        assert d[0][1:] == (None, []) and d[1][1:] == (None, [3])
        if n // 2 > 169:                                                         # 169 = 128 + 32 + 8 + 1
            assert d[169][1:] == (None, [e(1), e(8), e(32), e(128)]) and d[-169][2] == [e(-1), e(-8), e(-32), e(-128)]
            assert own[169][1:] == (None, [e(169)]) and own[-169][1:] == (None, [e(-169)])
        assert own[5][1:] == (None, [e(5)]) and own[-7][1:] == (None, [e(-7)]) and own[7][2] == [e(-1), e(8)]
        for rows in (d, own, plans[("empty", n)], plans[("columns", n)]):
            for s in (n // 2, -n // 2, n // 2 + 1, -n // 2 - 1):
                assert rows[s] == (0, TOO_LARGE, [])
            assert rows[0] == (2 * n - 1, None, [])
        for name in ("empty", "columns"):                                        # a power of two without its key: no further split
            for s in (1, -1, 4, -64, n // 4):
                assert plans[(name, n)][s][1] == NO_KEY
            assert plans[(name, n)][7][1] == NO_KEY and plans[(name, n)][n // 2 - 1][1] == NO_KEY
        assert d[n // 2 - 1][1:] == (None, [e(-1)])                           # N/2 - 1 has the element of -1: its own key


def test_rotation_header_is_clean_under_the_sanitizers(plans):
    """-fsanitize=undefined,address with errors fatal over the same sets: the same plans, no report"""
    r = run(build(("-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-g")))
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()[-2000:]
    assert parse(r.stdout.decode()) == plans
