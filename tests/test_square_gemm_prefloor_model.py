"""One fast floor per dense OUTPUT (cn_square_gemm's pre-floor form) in Python integers, and its bound function against exact arithmetic.  CPU only.

The per-input floor (k_behz_floor_f64) computes for one coefficient of one component of product k, from the tensor's residues x_kj = d_k mod q_j and x_kb = d_k mod b:
    y_kj = [x_kj t (q/q_j)^-1]_{q_j}  (canonical),    f_kb = T_b x_kb + sum_j N_bj y_kj  (mod b),    T_b = t q^-1,  N_bj = -(q/q_j) q^-1  (mod b)
and f_kb = W_k mod b for the integer W_k = floor(t d_k / q) - beta_k (bigint_model.behz_floor); Shenoy-Kumaresan turns the residues over Bsk into W_k mod q_j, the
word it writes.  The dense layer behind it forms sum_k w_k out_kj mod q_j.  The pre-floor form instead sums first - X_b = sum_k w_k x_kb mod b and the EXACT integer
Y_j = sum_k w_k y_kj - and runs one tail on f_b = T_b X_b + sum_j N_bj Y_j.  Checked here: SK(sum_k w_k f_k) == sum_k w_k out_k (mod q_j) for the moduli of the "tiny"
ring and its auxiliary base, tensor values with residues 0, q_j - 1 and q_j / 2, negative and zero weights, a bias on top; that every f_kb is W_k mod b; and that one
mutation - a y taken in another representative (y + q_j) - changes the result: y must stay canonical per input, only its weighted sum may be formed late.

cn_prefloor_bound_ok (cn_policy.h; tests/cpp/prefloor_bound.cpp) is one-sided: true implies 8 R t N q <= B m_sk / 2 (the exact inequality 4 R t N q < B m_sk / 2
with a bit to spare) and R q_j < 2^63.  Checked over a grid of (R, t, N, q, base) with R one bit either side of the edge: never true where the inequality fails,
always true a bit inside."""
import os
import random
import subprocess
import tempfile

import pytest

from bigint_model import add_plain, behz_floor, product
from conftest import PARAMS
from test_fp64_headroom import aux_primes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 256
Q = PARAMS["tiny"]["q"]
T = PARAMS["tiny"]["t"]
BSK = aux_primes(PARAMS["tiny"]["n"], len(Q) + 1)                     # B = the first k, m_sk the last


def floor_operands(d, canonical=True, bump=None):
    """(x_b over Bsk, y_j over q) of the tensor value d; bump = j: y_j in the representative y_j + q_j"""
    Qp = product(Q)
    y = [(d % qj) * T * pow(Qp // qj, -1, qj) % qj for qj in Q]
    if bump is not None:
        y[bump] += Q[bump]
    return [d % b for b in BSK], y


def f_of(x, y):
    """the floor's Bsk values from (X_b, Y_j): any integers Y_j"""
    Qp = product(Q)
    return [(T * pow(Qp, -1, b) * xb - sum((Qp // qj) * pow(Qp, -1, b) * yj for qj, yj in zip(Q, y))) % b for b, xb in zip(BSK, x)]


def shenoy_kumaresan(f):
    """residues over B and m_sk -> the centred integer they stand for (exact for |V| < B m_sk / 2 up to the conversion's own slack), per q_j"""
    B, msk = BSK[:-1], BSK[-1]
    Bp = product(B)
    S = sum((fl * pow(Bp // b, -1, b) % b) * (Bp // b) for fl, b in zip(f, B))
    alpha = (S - f[-1]) * pow(Bp, -1, msk) % msk
    if alpha > msk // 2:
        alpha -= msk
    V = S - alpha * Bp
    return V, [V % qj for qj in Q]


def tensor_values(rng, count):
    """tensor coefficients |d| <= 2 N q^2, the first ones with extreme residues mod every q_j: 0, q_j - 1 (d = -1 + m q), and q_j / 2 (by CRT)"""
    Qp = product(Q)
    lim = 2 * N * Qp * Qp
    half = sum((qj // 2) * (Qp // qj) * pow(Qp // qj, -1, qj) for qj in Q) % Qp
    d = [0, -1, Qp - 1, -1 + rng.randrange(-lim // Qp, lim // Qp) * Qp, rng.randrange(-lim // Qp, lim // Qp) * Qp, half, half - Qp * rng.randrange(lim // Qp), lim, -lim]
    return (d + [rng.randrange(-lim, lim + 1) for _ in range(count)])[:max(count, len(d))]


def weights(rng, count, wmax):
    w = [rng.randrange(-wmax, wmax + 1) for _ in range(count)]
    w[0], w[1], w[2] = wmax, -wmax, 0
    return w


@pytest.mark.parametrize("seed,wmax", [(1, 1), (2, 127), (3, 6144), (4, 32639)])
def test_one_floor_per_output_gives_the_words_of_one_floor_per_input(seed, wmax):
    rng = random.Random(0x9F100 + seed)
    d = tensor_values(rng, 40)
    w = weights(rng, len(d), wmax)
    W = [behz_floor(v, Q, T) for v in d]
    ops = [floor_operands(v) for v in d]
    for v, (x, y), Wk in zip(d, ops, W):
        assert f_of(x, y) == [Wk % b for b in BSK]                  # the per-input floor's Bsk values are W_k mod b
        assert shenoy_kumaresan(f_of(x, y))[1] == [Wk % qj for qj in Q]
    want = [sum(wk * (Wk % qj) for wk, Wk in zip(w, W)) % qj for qj in Q]
    X = [sum(wk * x[i] for wk, (x, _) in zip(w, ops)) % b for i, b in enumerate(BSK)]
    Y = [sum(wk * y[j] for wk, (_, y) in zip(w, ops)) for j in range(len(Q))]
    assert max(abs(v) for v in Y) < 2 ** 63
    V, got = shenoy_kumaresan(f_of(X, Y))
    assert V == sum(wk * Wk for wk, Wk in zip(w, W))
    assert got == want
    # the bias goes on top of either form's words alike (component 0; Delta m + the rounding term, bigint_model.add_plain)
    plain = [rng.randrange(T)]
    as_ct = lambda words: [[[x] for x in words], [[0] for _ in Q]]
    assert add_plain(as_ct(got), plain, Q, T) == add_plain(as_ct(want), plain, Q, T)


def test_a_y_in_another_representative_is_caught():
    rng = random.Random(0x9F1BAD)
    d = tensor_values(rng, 12)
    w = weights(rng, len(d), 127)
    W = [behz_floor(v, Q, T) for v in d]
    want = [sum(wk * (Wk % qj) for wk, Wk in zip(w, W)) % qj for qj in Q]
    for bad in (0, 5, len(d) - 1):                                   # (weights 127, != 0)
        if not w[bad]:
            continue
        ops = [floor_operands(v, bump=1 if i == bad else None) for i, v in enumerate(d)]
        X = [sum(wk * x[i] for wk, (x, _) in zip(w, ops)) % b for i, b in enumerate(BSK)]
        Y = [sum(wk * y[j] for wk, (_, y) in zip(w, ops)) for j in range(len(Q))]
        assert shenoy_kumaresan(f_of(X, Y))[1] != want


# ------------------------------------------------------------------ the bound function
def bound_cases():
    q44 = [0xffffffd8001, 0xffffffc8001, 0xfffff9a8001, 0xfffff8f8001, 0xfffff7c8001]                  # five 44-bit moduli (the size of the CryptoNets ring's)
    rings = [(PARAMS["tiny"]["n"], T, Q, aux_primes(1024, 4)),
             (4096, 40961, Q[:2], aux_primes(4096, 3)),
             (8192, PARAMS["c3"]["t"], q44, aux_primes(8192, 6)),
             (8192, 557057, q44, aux_primes(8192, 6)),
             (8192, PARAMS["c3"]["t"], q44, aux_primes(8192, 6)[:5] + [(1 << 61) - 1]),
             (2048, 12289, [0x3fffffff000001, 0x3fffffff004001], aux_primes(2048, 3))]
    out = []
    for n, t, q, base in rings:
        edge = product(base) // (16 * t * n * product(q))            # the largest R with 8 R t N q <= B m_sk / 2
        for R in {1, 18596, edge // 4, edge // 2, edge, edge + 1, 2 * edge, 4 * edge + 3, (2 ** 63 - 1) // max(q), (2 ** 63 - 1) // max(q) + 1, 0}:
            if 0 <= R < 2 ** 64:
                out.append((R, t, n, tuple(q), tuple(base)))
    return out


def test_bound_function_is_one_sided_and_not_idle():
    cases = bound_cases()
    d = tempfile.mkdtemp()
    exe, path = os.path.join(d, "prefloor_bound"), os.path.join(d, "cases.txt")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "prefloor_bound.cpp"), "-o", exe])
    with open(path, "w") as f:
        for R, t, n, q, base in cases:
            f.write("%d %d %d %d %s %d %s\n" % (R, t, n, len(q), " ".join(map(str, q)), len(base), " ".join(map(str, base))))
    ans = [bool(int(x)) for x in subprocess.run([exe, path], stdout=subprocess.PIPE, check=True, timeout=60).stdout.decode().split()]
    assert len(ans) == len(cases)
    seen = {True: 0, False: 0}
    for (R, t, n, q, base), a in zip(cases, ans):
        lhs, rhs, fits = 16 * R * t * n * product(q), product(base), R * max(q) < 2 ** 63
        if a:
            assert R > 0 and lhs <= rhs and fits, (R, t, n)          # one-sided: true implies the inequality, a bit to spare included
        if R > 0 and 2 * lhs <= rhs and fits:
            assert a, (R, t, n)                                      # a further bit inside it never refuses
        seen[a] += 1
    assert seen[True] and seen[False]
    c3 = [c for c in cases if c[0] == 18596 and c[2] == 8192 and c[1] == PARAMS["c3"]["t"] and max(c[4]) < 2 ** 49]
    assert c3 and all(ans[cases.index(c)] for c in c3)                # the shipped 845 -> 100 layer (R = 18 596) is inside
