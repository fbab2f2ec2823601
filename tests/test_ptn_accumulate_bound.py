"""cn_ptn_term_bound and cn_ptn_sum_interval (cryptonets_amd/csrc/cn_policy.h) - how many terms the lazy FP64 accumulators of k_mul_ptn_sum take between two
recentrings - against Python integers, for every modulus width from 30 to 49 bits.

A term is ArF64T::mulmod(x, w) of two canonical words below q: r = x w - h q exactly, with h = rint(fl(fl(x w) fl(1/q))).  Three roundings of relative error
2^-53 each put h within 1/2 + 3 (x w / q) 2^-53 < 1/2 + 3 q 2^-53 of x w / q, so |r| <= q/2 + 3 q^2 / 2^53: the bound the header derives, rounded up to an
integer (+ 1).  The interval is the largest count with count x bound < 2^52 - a recentred accumulator adds at most q/2 + 1 < 2^49, so no partial sum reaches 2^53 -
unless the cap (2^16) is lower, which the function reports.  The first assertion checks that bound against the arithmetic itself (exact rationals of the three
roundings at the worst operands); the others check the header.  tests/cpp/ptn_accumulate_bound.cpp is a plain g++ program: no device; it runs once more under
-fsanitize=undefined,address."""
import os
import subprocess
import tempfile
from fractions import Fraction

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 1 << 16


def moduli():
    """per width 30 .. 49: the smallest and the largest odd value of that width, and one in between; and 2^49.4, the largest modulus the FP64 tables admit"""
    qs = []
    for bits in range(30, 50):
        lo, hi = (1 << (bits - 1)) + 1, (1 << bits) - 1
        qs += [lo, (lo + hi) // 2 | 1, hi]
    return qs + [int(2 ** 49.4) | 1]


def bound_of(q):
    return q // 2 + 1 + -((-3 * q * q) >> 53)


def run(flags, d):
    exe, path = os.path.join(d, "ptn_accumulate_bound" + ("_san" if flags else "")), os.path.join(d, "moduli.txt")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", *flags, os.path.join(ROOT, "tests", "cpp", "ptn_accumulate_bound.cpp"), "-o", exe])
    with open(path, "w") as f:
        for q in moduli():
            f.write("%d\n" % q)
    out = subprocess.run([exe, path], stdout=subprocess.PIPE, check=True, timeout=60).stdout.decode().split("\n")
    rows = [tuple(int(x) for x in line.split()) for line in out if line.strip()]
    assert [r[0] for r in rows] == moduli()
    return {q: (b, i, bool(c)) for q, b, i, c in rows}


@pytest.fixture(scope="module")
def answers():
    d = tempfile.mkdtemp()
    return run([], d), d


def test_the_derived_bound_covers_the_three_roundings():
    """|x w / q - h| for the quotient estimate at its worst: every rounding off by a full relative 2^-53 in the same direction, x = w = q - 1"""
    u = Fraction(1, 2 ** 53)
    for q in moduli():
        exact = Fraction((q - 1) * (q - 1), q)
        worst = exact * (1 + u) ** 3                                  # fl(fl(x w) fl(1/q)) at most this far from x w / q
        err = worst - exact + Fraction(1, 2)                          # ... and rint moves it by at most 1/2
        assert err * q <= bound_of(q), q                              # |r| = q |x w / q - h|


def test_term_bound_and_interval_match_python_integers(answers):
    for q, (b, i, capped) in answers[0].items():
        assert b == bound_of(q), q
        fit = (2 ** 52 - 1) // b
        assert capped == (fit > CAP) and i == min(fit, CAP), (q, i, fit)
        assert i >= 1 and i * b < 2 ** 52, q                          # the interval fits ...
        if not capped:
            assert (i + 1) * b >= 2 ** 52, q                          # ... and one term more does not, where the function says it is the bound that limits it
        assert i * b + q // 2 + 1 < 2 ** 53, q                        # with the recentred accumulator underneath: still an exact integer in a double


def test_the_figures_the_kernel_comment_quotes(answers):
    a = answers[0]
    q49 = (1 << 49) - 1
    assert a[q49][1] == 11 and Fraction(a[q49][0], q49) < Fraction(69, 100)            # 0.69 q at 49 bits: 11 terms
    assert a[(1 << 47) - 1][1] == 58
    assert a[(1 << 30) - 1][2] is True and a[(1 << 30) - 1][1] == CAP                  # small moduli: the cap


def test_same_answers_under_the_sanitizers(answers):
    assert run(["-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-g"], answers[1]) == answers[0]
