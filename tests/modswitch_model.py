"""Models of BFV modulus switching (SEAL 3.2 Evaluator.mod_switch_scale_to_next, applied once per dropped prime) - test infrastructure, CPU only.

Two independent statements of one drop of the last prime q_l of q = (q_0 .. q_l):
  bigint    the CRT value x in [0, Q) of a coefficient, x' = floor((x + floor(q_l / 2)) / q_l) mod Q' (Q' = Q / q_l), on Python integers;
  residues  SEAL's residue formula: r = (x_l + h) mod q_l, x_i' = (x_i - (r mod q_i) + (h mod q_i)) q_l^-1 mod q_i.
A switch by several primes is SUCCESSIVE single drops (SEAL's mod_switch_to loops), not one rounding by their product.
"""
import numpy as np


def crt_compose(res, q):
    """residues (one per modulus) -> x in [0, prod q)"""
    Q = 1
    for m in q:
        Q *= m
    x = 0
    for r, m in zip(res, q):
        Qi = Q // m
        x += int(r) * Qi * pow(Qi, -1, m)
    return x % Q


def drop_bigint(x, q):
    """one drop of q[-1] on the CRT value x of q -> CRT value over q[:-1]"""
    ql = q[-1]
    Qp = 1
    for m in q[:-1]:
        Qp *= m
    return ((x + ql // 2) // ql) % Qp


def switch_bigint(x, q, limbs):
    for p in range(len(q), limbs, -1):
        x = drop_bigint(x, q[:p])
    return x


def switch_residues(words, q, n, limbs):
    """ciphertext words [size][k][N] (any leading shape flattened) over q -> words [size][limbs][N] over q[:limbs], by SEAL's residue formula"""
    k = len(q)
    a = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, k, n)
    x = [a[:, j].astype(object) for j in range(k)]
    for p in range(k - 1, limbs - 1, -1):
        ql = q[p]
        h = ql // 2
        r = (x[p] + h) % ql
        for i in range(p):
            qi = q[i]
            x[i] = ((x[i] - r % qi + h % qi) * pow(ql, -1, qi)) % qi
    out = np.stack([x[i].astype(np.uint64) for i in range(limbs)], axis=1)
    return out.reshape(-1)


def slice_key(words, k, n, digits, limbs):
    """a key-switch key of a context over q[:k] ([entries (l, d)][2][k][N], entries in (l, d) order, digits[l] per limb) -> the level's key:
    entries with l < limbs, each the first `limbs` limbs of both polynomials"""
    w = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, 2, k, n)
    keep = sum(digits[:limbs])
    return np.ascontiguousarray(w[:keep, :, :limbs]).reshape(-1)


def slice_poly(words, k, n, limbs, polys):
    """public key (polys = 2) / secret key (polys = 1) [polys][k][N] -> [polys][limbs][N]"""
    w = np.ascontiguousarray(words, dtype=np.uint64).reshape(polys, k, n)
    return np.ascontiguousarray(w[:, :limbs]).reshape(-1)


def digits(q, dbc):
    """base-2^dbc digits of a residue mod each q_j"""
    return [(m.bit_length() + dbc - 1) // dbc for m in q]
