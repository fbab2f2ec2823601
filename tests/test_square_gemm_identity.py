"""The identity cn_square_gemm rests on, in plain integers (CPU only, no library code).

SquareActivation relinearizes every product, ct_k = (d0_k + KS0(d2_k), d1_k + KS1(d2_k)), and the dense layer behind it forms
out_o = sum_k w_ok ct_k.  A key switch cuts its operand into base-2^dbc digits - the only non-linear step - and everything behind that
(evaluation at the roots, the products with the key, the reduction mod q_j) is linear over Z_{q_j}, as is the weighted sum.  So

    sum_k w_ok KSc(d2_k)[j]  ==  sum_{l,d} eval_j(S_{o,l,d}) K^c_{l,d,j}   with   S_{o,l,d} = sum_k w_ok digit_{l,d}(d2_k)   (a plain integer)

word for word: one key switch per OUTPUT, fed with the weight-combined digit polynomials.  Checked here at N = 64 with the reference's
coefficient moduli (CoeffModulus128(8192), dbc 10) in the evaluation domain of tests/bigint_model.py - N values at N distinct points pin
every word of a limb.  Keys are random words: the identity does not depend on what the key encrypts.  Taking the digits of the SUM
instead (relinearizing late) must NOT give these words: the mutation check.
"""
import random

import bigint_model as bm

N, DBC = 64, 10
Q = [0x7fffffd8001, 0x7fffffc8001, 0xfffffffc001, 0xffffff6c001, 0xfffffebc001]          # CoeffModulus128(8192) of the reference's SEAL: 43, 43, 44, 44, 44 bits
T = 549764251649
WMAX = (1 << 20) - 1


def setup_module(module):
    for qj in Q:
        assert (qj - 1) % (2 * N) == 0


def digit_count(q):
    return [-(-qj.bit_length() // DBC) for qj in q]


def random_key(rng, q):
    """flat [(l, d)][2][k][N] words below q_j (bigint_model.key_switch_eval's layout)"""
    words = []
    for _ in range(sum(digit_count(q))):
        for _c in range(2):
            for qj in q:
                words += [rng.randrange(qj) for _ in range(N)]
    return words


def products(rng, q, count):
    """`count` size-3 products [3][k][N]; the first three with residues at the edges of the range in d2"""
    out = []
    for c in range(count):
        ct = [[[rng.randrange(qj) for _ in range(N)] for qj in q] for _ in range(3)]
        if c == 0:
            ct[2] = [[qj - 1] * N for qj in q]
        elif c == 1:
            ct[2] = [[0] * N for _ in q]
        elif c == 2:
            ct[2] = [[(1 << (qj.bit_length() - 1)) - 1 if i % 2 else qj // 2 for i in range(N)] for qj in q]       # all digits full / the middle
        out.append(ct)
    return out


def centred(w):
    return w - T if w >= (T + 1) // 2 else w


def relinearize_then_sum(prods, rows, key, q, pts):
    """form A, in the evaluation domain: values of out_o[c][j] = sum_k w_ok (d_c,k + KSc(d2_k)) at the N points of limb j"""
    k = len(q)
    per_ct = []
    for ct in prods:
        acc, _ = bm.key_switch_eval(ct[2], key, q, DBC, N)
        per_ct.append([[[(e + a) % qj for e, a in zip(bm.evaluate(ct[c][j], pts[j], qj), acc[c][j])] for j, qj in enumerate(q)] for c in range(2)])
    out = []
    for row in rows:
        out.append([[[sum(centred(w) * per_ct[kk][c][j][p] for kk, w in enumerate(row) if w) % q[j] for p in range(N)] for j in range(k)] for c in range(2)])
    return out


def key_switch_of_digits(digit_polys, key, q, pts):
    """sum over the (limb, digit) polynomials - plain (signed) integers, the same for every output limb - of eval_j(poly) x key: acc[c][j][p]"""
    k = len(q)
    acc = [[[0] * N for _ in range(k)] for _ in range(2)]
    for g, poly in enumerate(digit_polys):
        for j, qj in enumerate(q):
            vals = bm.evaluate([v % qj for v in poly], pts[j], qj)
            for c in range(2):
                base = ((g * 2 + c) * k + j) * N
                for p in range(N):
                    acc[c][j][p] = (acc[c][j][p] + vals[p] * key[base + p]) % qj
    assert len(key) == len(digit_polys) * 2 * k * N
    return acc


def combined_digits(prods, row, q):
    """S_{l,d} = sum_k w_k digit_{l,d}(d2_k): digits FIRST, then the weights"""
    out = []
    for l, ql in enumerate(q):
        per_in = [bm.digits_of(ct[2][l], ql, DBC) for ct in prods]
        for d in range(len(per_in[0])):
            out.append([sum(centred(w) * per_in[kk][d][i] for kk, w in enumerate(row) if w) for i in range(N)])
    return out


def digits_of_the_sum(prods, row, q):
    """the mutation: weights first (mod q_l), THEN the digits - what relinearizing the weighted sum of size-3 products would decompose"""
    out = []
    for l, ql in enumerate(q):
        s = [sum(centred(w) * ct[2][l][i] for kk, (w, ct) in enumerate(zip(row, prods)) if w) % ql for i in range(N)]
        out += bm.digits_of(s, ql, DBC)
    return out


def sum_then_switch(prods, rows, key, q, pts, digits):
    """form B: values of (sum_k w_ok d_c,k) + KSc(from `digits`) at the points"""
    out = []
    for row in rows:
        acc = key_switch_of_digits(digits(prods, row, q), key, q, pts)
        lin = [[[sum(centred(w) * ct[c][j][i] for w, ct in zip(row, prods) if w) % qj for i in range(N)] for j, qj in enumerate(q)] for c in range(2)]
        out.append([[[(e + a) % qj for e, a in zip(bm.evaluate(lin[c][j], pts[j], qj), acc[c][j])] for j, qj in enumerate(q)] for c in range(2)])
    return out


def weight_rows(rng, K):
    res = lambda v: v % T
    return [[res(rng.randrange(-WMAX, WMAX + 1)) for _ in range(K)],                              # random
            [res(WMAX if kk % 2 else -WMAX) for kk in range(K)],                                  # the extremes, alternating
            [res(WMAX)] * K,                                                                       # the largest row sum
            [0 if kk % 3 else res(-WMAX) for kk in range(K)]]                                     # zeros skip their terms


def test_key_switch_of_combined_digits_is_the_sum_of_key_switches():
    rng = random.Random(0x5147)
    K = 5
    q = Q
    assert K * WMAX * ((1 << DBC) - 1) < min(q) // 2 and K * WMAX * ((1 << DBC) - 1) < 1 << 52         # |S| stays a recentred exact double
    pts = [bm.eval_points(N, qj) for qj in q]
    key, prods, rows = random_key(rng, q), products(rng, q, K), weight_rows(rng, K)
    want = relinearize_then_sum(prods, rows, key, q, pts)
    got = sum_then_switch(prods, rows, key, q, pts, combined_digits)
    assert got == want
    for row in rows:                                                                               # and S is what the bound says
        assert max(abs(v) for poly in combined_digits(prods, row, q) for v in poly) <= K * WMAX * ((1 << DBC) - 1)


def test_digits_taken_after_the_sum_are_caught():
    rng = random.Random(0x5148)
    K, q = 3, Q[:2]
    pts = [bm.eval_points(N, qj) for qj in q]
    key, prods, rows = random_key(rng, q), products(rng, q, K), weight_rows(rng, K)[:2]
    want = relinearize_then_sum(prods, rows, key, q, pts)
    assert sum_then_switch(prods, rows, key, q, pts, combined_digits) == want
    assert sum_then_switch(prods, rows, key, q, pts, digits_of_the_sum) != want
