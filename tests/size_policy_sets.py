"""One prime set per arithmetic policy (cn_policy.h) that serves every register-radix ring, N = 1024 .. 16384 - test infrastructure, no device at import.

The primes are the largest below 2^bits that are 1 mod 32768 (ntt_primes of test_gpu_wide_moduli): valid for every N <= 16384.  Limb sizes
    u64   60, 60, 50 bits   one limb of 50 bits or more: ArU64 (Shoup) everywhere, SEAL's 61-bit auxiliary base
    f64   49, 49, 47 bits   below 2^49, above 44 bits: ArF64 (forward recentring, lazy accumulators recentred every other term)
    f64l  44, 40, 36 bits   at most 44 bits: ArF64L
k = 3, t = 65537 (1 mod 2N for every size).  A cell is (policy, N); every cell exists at two digit widths, dbc = gdbc = 60 (one digit per limb) and
dbc = gdbc = 10 (17, 15 and 13 digits: at 12 or more the fused key switch keeps its forward twiddles in LDS at N <= 8192, the digit sums of the
one-key-switch-per-output calls are int32 words, N = 16384 runs the multi-digit k_keyswitch_pair14).

SETS holds the 15 cells under the names tests/test_policy_table.py prints (one width: the policy of a range does not depend on the digit width).
Cell is what a GPU test works on: the oracle with its keys, a device context with the relinearisation key and the Galois keys of STEPS and the column swap.
"""
import numpy as np

from modswitch_model import digits, slice_key, slice_poly
from test_gpu_wide_moduli import ntt_primes

T = 65537
SIZES = (1024, 2048, 4096, 8192, 16384)
POLICIES = ("u64", "f64", "f64l")
WIDTHS = (60, 10)
BITS = {"u64": (60, 60, 50), "f64": (49, 49, 47), "f64l": (44, 40, 36)}
STEPS = (1, -1, -2, -4)                                     # the row rotations a test may ask for in one hop (sum_slots of length 8: -1, -2, -4)


def primes(policy):
    out = []
    for b in BITS[policy]:
        out.append(ntt_primes(b, 16384, 1, avoid=out)[0])
    return out


Q = {p: primes(p) for p in POLICIES}
for _p in POLICIES:
    assert [m.bit_length() for m in Q[_p]] == list(BITS[_p]) and len(set(Q[_p])) == 3 and all(m % 32768 == 1 for m in Q[_p])
assert all(T % (2 * n) == 1 for n in SIZES)

CELLS = [(p, n) for p in POLICIES for n in SIZES]
NAME = lambda policy, n: "sp-%s-n%d" % (policy, n)
SETS = {NAME(p, n): dict(n=n, t=T, q=Q[p], dbc=60, gdbc=60) for p, n in CELLS}
DIGITS = {p: {w: sum(digits(Q[p], w)) for w in WIDTHS} for p in POLICIES}
assert DIGITS == {"u64": {60: 3, 10: 17}, "f64": {60: 3, 10: 15}, "f64l": {60: 3, 10: 13}}


class Cell:
    """(policy, N, digit width): oracle with keys, device context with the relinearisation key and the Galois keys of STEPS and the column swap"""

    def __init__(self, policy, n, width, seed=23):
        from cryptonets_amd._native import Context
        from oracle.cno import Oracle
        self.policy, self.n, self.width, self.q = policy, n, width, list(Q[policy])
        self.o = Oracle(n, T, q=self.q, dbc=width, gdbc=width)
        self.o.keygen(seed, galois=True)
        self.g = Context(n, T, q=self.q, dbc=width, gdbc=width, device=0)
        self.g.set_relin_key(self.o.relin_key())
        have = self.o.galois_elts()
        self.elts = [self.o.galois_elt_from_step(s) for s in STEPS] + [2 * n - 1]
        for e in self.elts:
            self.g.set_galois_key(e, self.o.galois_key(have.index(e)))
        self.tot = DIGITS[policy][width]                      # digits of a key switch (relinearisation and Galois alike: dbc = gdbc)
        self._level = None

    def level(self, limbs=2):
        """(oracle over q[:limbs] with the sliced keys, the device's level context) - made once, after the keys were uploaded"""
        from oracle.cno import Oracle
        if self._level is None:
            o, w = self.o, self.width
            lo = Oracle(self.n, T, q=self.q[:limbs], dbc=w, gdbc=w)
            lo.import_keys(slice_poly(o.secret_key(), o.k, o.n, limbs, 1), slice_poly(o.public_key(), o.k, o.n, limbs, 2))
            lo.import_relin_key(slice_key(o.relin_key(), o.k, o.n, digits(o.q, w), limbs))
            have = o.galois_elts()
            for e in self.elts:
                lo.import_galois_key(e, slice_key(o.galois_key(have.index(e)), o.k, o.n, digits(o.q, w), limbs))
            self._level = (lo, self.g.level(limbs))
        return self._level

    def close(self):
        for lv in list(self.g._levels.values()):            # a level context outlives its parent: each is released on its own
            lv.close()
        self.g.close()


def uniform(o, rng, count, size=2):
    """`count` ciphertexts of `size` polynomials, every word uniform below its modulus"""
    return np.stack([np.concatenate([rng.integers(0, m, size=o.n, dtype=np.uint64) for _ in range(size) for m in o.q]) for _ in range(count)])


def edge_words(o, rng, count, size=2):
    """uniform ciphertext words with the edge residues 0, 1, (q - 1) / 2, (q + 1) / 2 and q - 1 planted: ciphertext 0 cycles through the five in every limb
    (shifted by the limb and the polynomial), ciphertext 1 is q - 1 everywhere, every other one carries the five at its first and last coefficients"""
    X = uniform(o, rng, count, size)
    w = X.reshape(count, size, o.k, o.n)
    for j, m in enumerate(o.q):
        e = np.array([0, 1, (m - 1) // 2, (m + 1) // 2, m - 1], dtype=np.uint64)
        for p in range(size):
            w[0, p, j] = e[(np.arange(o.n) + j + p) % 5]
            if count > 1:
                w[1, p, j] = m - 1
            for c in range(2, count):
                w[c, p, j, :5] = e
                w[c, p, j, -5:] = e[::-1]
    return X
