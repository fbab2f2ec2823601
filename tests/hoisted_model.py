"""The word contract of the hoisted rotations (cn_rotate_rows_hoisted / cn_apply_galois_hoisted, include/cnhip.h) in Python integers - test infrastructure, no device.

For an input (c0, c1), an odd element g < 2N and its Galois key K_g[(l,d)][p][j] (NTT form, entries in (l, d) order):

    D_(l,d)[i]          = digit d (base 2^gdbc, low to high) of c1 limb l, coefficient i          (ks_xi: of [c1_l (q/q_l)^-1]_(q_l))
    s_g(D)_j[i g mod N] = +- (D[i] mod q_j), negative when (i g mod 2N) >= N                       (canonical)
    out_p limb j        = INTT_j( sum_(l,d) NTT_j(s_g(D_(l,d))_j) . K_g[(l,d)][p][j] )  +  (p == 0 ? s_g(c0)_j : 0)

These are NOT SEAL's words: SEAL permutes c1 first and cuts digits afterwards, and a negated coefficient q_l - x has other digits than x.  The plaintext is the
same and the key-switch noise is a sum over the same digits against the same key errors, permuted.  The transforms are the oracle's (Oracle.ntt_fwd / ntt_inv),
the products and sums are Python integers.

The device never forms s_g(D): it uses NTT_j(s_g(D)) = P_g(NTT_j(D mod q_j)) with P_g a pure permutation of the transform's output (perm_index), which
tests/test_hoisted_model.py checks against the oracle's transform before any kernel relies on it."""
import numpy as np

from modswitch_model import digits


def brev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2)


def perm_index(n, g):
    """src with NTT(s_g(a))[p] = NTT(a)[src[p]] in SEAL's output order: position p holds the evaluation at psi^(2 brev(p) + 1), which x -> x^g takes to the
    evaluation at psi^((2 brev(p) + 1) g mod 2N)"""
    bits = n.bit_length() - 1
    return np.array([brev((((2 * brev(p, bits) + 1) * g) % (2 * n) - 1) // 2, bits) for p in range(n)], dtype=np.int64)


def automorphism(a, g, q):
    """s_g of a coefficient-form polynomial mod q: out[i g mod N] = +- a[i], negative when (i g mod 2N) >= N; canonical"""
    n = len(a)
    i = np.arange(n, dtype=np.int64)
    pos = (i * int(g)) % (2 * n)
    a = np.array([int(x) % q for x in a], dtype=np.uint64) if np.asarray(a).dtype == object else np.asarray(a, dtype=np.uint64) % np.uint64(q)
    out = np.zeros(n, dtype=np.uint64)
    out[pos % n] = np.where(pos >= n, (np.uint64(q) - a) % np.uint64(q), a)
    return out


def digit_polys(o, c1, ks_xi=False):
    """[(l, d, D)]: the digit polynomials of c1 ([k][N] words), plain integers below 2^gdbc, in the key's entry order"""
    Q = 1
    for m in o.q:
        Q *= m
    out = []
    for l, m in enumerate(o.q):
        x = np.asarray(c1[l], dtype=object)
        if ks_xi:
            x = (x * pow(Q // m, -1, m)) % m
        for d in range(digits(o.q, o.gdbc)[l]):
            out.append((l, d, ((x >> (o.gdbc * d)) & ((1 << o.gdbc) - 1)).astype(np.uint64)))
    return out


def hoisted(o, ct, g, key, ks_xi=False):
    """the words [2][k][N] (flattened, uint64) of the hoisted rotation of ct by the element g under the Galois key words `key` of g"""
    n, k = o.n, o.k
    w = np.ascontiguousarray(ct, dtype=np.uint64).reshape(2, k, n)
    if g == 1:
        return w.reshape(-1).copy()
    D = digit_polys(o, w[1], ks_xi)
    K = np.ascontiguousarray(key, dtype=np.uint64).reshape(len(D), 2, k, n)
    out = np.zeros((2, k, n), dtype=np.uint64)
    for j, m in enumerate(o.q):
        acc = [np.zeros(n, dtype=object), np.zeros(n, dtype=object)]
        for e, (_, _, dig) in enumerate(D):
            f = o.ntt_fwd(j, automorphism(dig, g, m)).astype(object)
            for p in range(2):
                acc[p] = acc[p] + f * K[e, p, j].astype(object)
        for p in range(2):
            r = o.ntt_inv(j, (acc[p] % m).astype(np.uint64)).astype(object)
            if p == 0:
                r = (r + automorphism(w[0, j], g, m)) % m
            out[p, j] = r.astype(np.uint64)
    return out.reshape(-1)
