"""cn_digit_sum_fits_i32 (cryptonets_amd/csrc/cn_policy.h) - the plan-level decision "the digit sums of this layer fit int32 words" - against Python integers.

gemm_digit_form (cn_gemm_plan.h) asks it with the largest sum_k |w_ok| of any output, cn_mul_relin_sum with K (unit weights): true iff sum (2^dbc - 1) <= 2^31 - 1.  The two boundary
values of the product, 2^31 - 1 and 2^31, are reached exactly only at dbc = 1 (2^31 - 1 is prime) and, for the lower one, at dbc = 31 with sum 1; every other
dbc is asked at the last sum that fits and the first that does not.  tests/cpp/digit_sum_bound.cpp is a plain g++ program: no device."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32_MAX = 2 ** 31 - 1


def cases():
    c = [(I32_MAX, 1), (I32_MAX + 1, 1), (1, 31), (2, 31), (0, 10), (1, 0), (1, 32), (1, 63), (2 ** 64 - 1, 1), (2 ** 64 - 1, 31), (2 ** 63, 2)]
    for dbc in range(1, 32):
        last = I32_MAX // (2 ** dbc - 1)
        c += [(last, dbc), (last + 1, dbc)]
    c += [(18596, 10), (845 * (2 ** 20 - 1), 10), (2 ** 21, 10), (2 ** 21 + 2 ** 11, 10), (2 ** 21 + 2 ** 11 + 1, 10)]      # the workload's 845 -> 100 layer; around 2^31 / 1023
    return c


@pytest.fixture(scope="module")
def answers():
    d = tempfile.mkdtemp()
    exe, path = os.path.join(d, "digit_sum_bound"), os.path.join(d, "cases.txt")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "digit_sum_bound.cpp"), "-o", exe])
    with open(path, "w") as f:
        for s, dbc in cases():
            f.write("%d %d\n" % (s, dbc))
    out = subprocess.run([exe, path], stdout=subprocess.PIPE, check=True, timeout=60).stdout.decode().split("\n")
    rows = [tuple(int(x) for x in line.split()) for line in out if line.strip()]
    assert [(s, dbc) for s, dbc, _ in rows] == cases()
    return {(s, dbc): bool(a) for s, dbc, a in rows}


def test_the_two_boundary_values(answers):
    assert I32_MAX * (2 ** 1 - 1) == 2 ** 31 - 1 and answers[(I32_MAX, 1)] is True
    assert (I32_MAX + 1) * (2 ** 1 - 1) == 2 ** 31 and answers[(I32_MAX + 1, 1)] is False
    assert 1 * (2 ** 31 - 1) == 2 ** 31 - 1 and answers[(1, 31)] is True and answers[(2, 31)] is False


def test_every_answer_matches_python_integers(answers):
    for (s, dbc), a in answers.items():
        want = 1 <= dbc <= 31 and s * (2 ** dbc - 1) <= I32_MAX
        assert a == want, (s, dbc, a)
    assert answers[(18596, 10)] is True                              # the shipped 845 -> 100 layer: 18 596 x 1023 < 2^25
