"""The oracle's ciphertext WORDS against independent big-integer mathematics (tests/bigint_model.py: no transform, no modular-arithmetic
tricks, no code shared with oracle/seal32_oracle.c).  VERDICT r02: until this file the oracle's multiply / relinearize / rotate /
multiply_plain / add_plain were checked at the decrypted-slot level only - a digit order, plain lift or rounding variant that still
decrypts correctly would have become the golden digest and the HIP path would have been held bit-exact to it.  Here such a variant fails
on the CPU: every assertion below is WORD equality (or, for key switches, equality of the result polynomial at all N evaluation points).

Sizes: add_plain and multiply_plain run at BASELINE config 2's full size (N = 8192, 2 limbs - SURVEY 8d: "expected = Python big-int
negacyclic product with SEAL's plain lift") and at config 3's five limbs; the BEHZ product, relinearisation and the Galois key
switches at N <= 256 with the reference's real moduli (SEAL's 61-bit auxiliary base in the oracle - the model needs none, its result
is base-independent by construction) including extreme operands."""
import numpy as np
import pytest

import bigint_model as M
from oracle.cno import COEFF_MODULUS_128, Oracle

Q8192 = COEFF_MODULUS_128[8192]
SMALL = [
    # (n, t, q, dbc, gdbc)
    (64, 257, [0xffffee001, 0xffffc4001, 0x1ffffe0001], 10, 20),            # CoeffModulus128(4096) - the default factory's limbs
    (64, 257, [0xffffee001, 0xffffc4001], 16, 60),                          # one digit per limb for Galois (dbc 60), three for relin
    (128, 12289, Q8192, 10, 20),                                            # CryptoNets / LoLa limbs and digit widths
    (256, 12289, Q8192[:2], 10, 20),                                        # config 2's limbs, Kronecker products in the model
    (32, 193, COEFF_MODULUS_128[16384][:8], 60, 60),                        # LoLa-CIFAR limbs (48-49 bits), dbc 60
    # 50-60-bit moduli: the integer transforms and key switch, SEAL's 61-bit auxiliary base (the widest moduli SEAL 3.2 accepts)
    (64, 257, [0xffffffffffe8001, 0xffffffffffd8001], 60, 60),              # two primes just below 2^60, one digit per limb
    (64, 257, [0xffffffffffe8001, 0xffffffffffd8001, 0xffffee001], 10, 20),  # beside a 36-bit prime: six 10-bit digits per wide limb
    (64, 257, [0x3fffffff000001, 0xffffffffffc0001], 59, 59),               # 54 and 60 bits: the top digit of the wide limb is 1 bit
]


def _oracle(n, t, q, dbc, gdbc, seed=7, galois=True, xi=False):
    o = Oracle(n, t, q=q, dbc=dbc, gdbc=gdbc, ks_xi=xi)
    o.keygen(seed, galois=galois)
    return o


# the two self-consistent decomposition conventions of the digit key switch (oracle gen_ksk, libcnhip "ks_xi"): SURVEY 9.5's raw-residue
# digits, and the xi_q form of the BEHZ paper.  SEAL's source is not on disk to say which one 3.2 ships, so both are restated, both are
# pinned to the big-integer model, and the product carries both behind a start-up self-test.
XI = pytest.mark.parametrize("xi", [False, True], ids=["raw-digits", "xi-digits"])


def _fresh(o, rng, hi=None):
    return o.encrypt(o.encode(rng.integers(0, hi or o.t, o.n, dtype=np.uint64)))


def _extreme_ct(o, kind):
    """ciphertext-shaped words at the edges of the residue range (not encryptions of anything: the evaluator's arithmetic must be exact
    on every input)"""
    w = np.zeros((2, o.k, o.n), dtype=np.uint64)
    for j, qj in enumerate(o.q):
        if kind == "max":
            w[:, j, :] = qj - 1
        elif kind == "half":
            w[0, j, :] = qj // 2
            w[1, j, :] = qj // 2 + 1
        elif kind == "alt":
            w[0, j, ::2] = qj - 1
            w[1, j, 1::2] = 1
    return w.reshape(-1)


# ---------------------------------------------------------------------------------------------------- linear operations
@pytest.mark.parametrize("q,t", [(Q8192[:2], 549764251649), (Q8192, 549764251649), (Q8192, 557057)], ids=["c2", "c3", "c4"])
def test_add_plain_words_full_size(q, t):
    """Delta-scaling with the upper-half increment, N = 8192 (AtomicSealBfvVector.cs:1019,1267)"""
    rng = np.random.default_rng(len(q) + t % 97)
    o = _oracle(8192, t, q, 10, 20, galois=False)
    ct = _fresh(o, rng)
    plain = rng.integers(0, t, o.n, dtype=np.uint64)
    plain[:6] = [0, 1, (t + 1) // 2 - 1, (t + 1) // 2, t - 1, t - 2]          # both sides of the upper-half threshold
    c = M.ct_limbs(ct, 2, o.k, o.n)
    for sub in (False, True):
        assert M.flatten(M.add_plain(c, plain, q, t, sub)) == [int(x) for x in o.add_plain(ct, plain, sub)]


@pytest.mark.parametrize("q,t", [(Q8192[:2], 549764251649), (Q8192, 549764251649)], ids=["c2", "c3"])
def test_multiply_plain_words_full_size(q, t):
    """BASELINE config 2 (one N = 8192, 2-limb ciphertext x plaintext) and config 3's limbs: dense product = negacyclic product with the
    fast plain lift, by Kronecker substitution over Python integers; constant and monomial plaintexts (the sparse-format weights of
    AtomicSealBfvVector.cs:1136 take SEAL's monomial path)"""
    rng = np.random.default_rng(2 + len(q))
    o = _oracle(8192, t, q, 10, 20, galois=False)
    ct = _fresh(o, rng)
    c = M.ct_limbs(ct, 2, o.k, o.n)
    dense = rng.integers(0, t, o.n, dtype=np.uint64)
    dense[:4] = [t - 1, (t + 1) // 2, (t + 1) // 2 - 1, 0]
    assert M.flatten(M.multiply_plain(c, dense, q, t)) == [int(x) for x in o.multiply_plain(ct, dense)]
    for const in (t - 5, 7, (t + 1) // 2):                                    # constant polynomials: negative, positive, threshold
        assert M.flatten(M.multiply_plain(c, [const], q, t)) == [int(x) for x in o.multiply_plain(ct, np.array([const], dtype=np.uint64))]
    mono = np.zeros(o.n, dtype=np.uint64)
    mono[4097] = t - 3                                                        # c x^e, e > N/2: wraps negacyclically
    assert M.flatten(M.multiply_plain(c, mono, q, t)) == [int(x) for x in o.multiply_plain(ct, mono)]
    ext = _extreme_ct(o, "max")
    assert M.flatten(M.multiply_plain(M.ct_limbs(ext, 2, o.k, o.n), dense, q, t)) == [int(x) for x in o.multiply_plain(ext, dense)]


# ---------------------------------------------------------------------------------------------------- BEHZ multiplication
@pytest.mark.parametrize("n,t,q,dbc,gdbc", SMALL, ids=lambda v: None)
def test_multiply_words_equal_the_exact_integer_characterisation(n, t, q, dbc, gdbc):
    """Evaluator.Multiply: (1) every operand coefficient is the integer Y = (X + q r) / m~ recovered from its q residues (m~ = 2^32, r
    centred), (2) integer negacyclic tensor, (3) W = floor(t d / q) - beta with beta the overshoot of the q-side fast base conversion,
    (4) W mod q_j.  Fresh encryptions, a squaring, and extreme residues."""
    rng = np.random.default_rng(n * 7 + len(q))
    o = _oracle(n, t, q, dbc, gdbc, galois=False)
    a, b = _fresh(o, rng), _fresh(o, rng)
    cases = [(a, b), (a, a), (_extreme_ct(o, "max"), _extreme_ct(o, "max")), (_extreme_ct(o, "half"), b), (_extreme_ct(o, "alt"), _extreme_ct(o, "half")),
             (np.zeros_like(a), b)]
    for x, y in cases:
        want = M.flatten(M.multiply(M.ct_limbs(x, 2, o.k, n), M.ct_limbs(y, 2, o.k, n), q, t))
        assert want == [int(v) for v in o.multiply(x, y)]


def test_behz_lift_is_congruent_and_bounded():
    """the model's own premise: Y == c mod every q_j and |Y| <= q (1/2 + k / m~) - so steps (2)-(4) see the integers BEHZ means"""
    q = Q8192
    Q = M.product(q)
    rng = np.random.default_rng(5)
    for _ in range(200):
        res = [int(rng.integers(0, qj)) for qj in q]
        Y = M.behz_lift(res, q)
        assert all(Y % qj == r for qj, r in zip(q, res))
        assert abs(Y) * M.M_TILDE * 2 <= Q * (M.M_TILDE + 2 * len(q))


# ---------------------------------------------------------------------------------------------------- key switching
@XI
@pytest.mark.parametrize("n,t,q,dbc,gdbc", SMALL, ids=lambda v: None)
def test_relinearize_words(n, t, q, dbc, gdbc, xi):
    """Evaluator.Relinearize: digits of every limb of c2, low -> high, times key (limb, digit), added to (c0, c1) - checked at all N
    evaluation points of every output limb.  Inputs: a real product and extreme size-3 words (digits 1023 / 0 patterns)."""
    rng = np.random.default_rng(n + dbc)
    o = _oracle(n, t, q, dbc, gdbc, galois=False, xi=xi)
    a, b = _fresh(o, rng), _fresh(o, rng)
    rk = o.relin_key()
    c3s = [o.multiply(a, b)]
    ext = np.zeros((3, o.k, n), dtype=np.uint64)
    for j, qj in enumerate(q):
        ext[:, j, :] = qj - 1
        ext[2, j, ::3] = (1 << dbc) - 1 if dbc < 60 else qj // 3
    c3s.append(ext.reshape(-1))
    for c3 in c3s:
        out = M.ct_limbs(o.relinearize(c3), 2, o.k, n)
        x = M.ct_limbs(c3, 3, o.k, n)
        M.assert_key_switched(out, x[0], x[1], x[2], rk, q, dbc, xi=xi)
    # and the product still means what it should: decrypt(relinearize(a b)) == decrypt(a) decrypt(b) slot by slot
    if o.L.cno_batching(o.h):
        want = (o.decode(o.decrypt(a)).astype(object) * o.decode(o.decrypt(b)).astype(object)) % t
        assert [int(v) for v in o.decode(o.decrypt(o.relinearize(c3s[0])))] == [int(v) for v in want]


def _check_galois(o, ct, out_words, elt, key):
    n, q = o.n, o.q
    c = M.ct_limbs(ct, 2, o.k, n)
    s0 = [M.galois_poly(c[0][j], elt, q[j]) for j in range(o.k)]
    s1 = [M.galois_poly(c[1][j], elt, q[j]) for j in range(o.k)]
    M.assert_key_switched(M.ct_limbs(out_words, 2, o.k, n), s0, None, s1, key, q, o.gdbc, xi=o.ks_xi)


@XI
@pytest.mark.parametrize("n,t,q,dbc,gdbc", SMALL[:4], ids=lambda v: None)
def test_apply_galois_and_rotation_words(n, t, q, dbc, gdbc, xi):
    """Evaluator.ApplyGalois = (sigma(c0) + KS(sigma(c1))_0, KS(sigma(c1))_1) with the element's key; RotateRows with a direct key, with a
    NAF-decomposed step count (successive +-2^i rotations, low-order first), RotateColumns (element 2N - 1)"""
    rng = np.random.default_rng(n + gdbc)
    o = _oracle(n, t, q, dbc, gdbc, xi=xi)
    elts = o.galois_elts()
    ct = _fresh(o, rng)
    for gi in (0, 1, len(elts) // 2, len(elts) - 1):
        _check_galois(o, ct, o.apply_galois(ct, elts[gi]), elts[gi], o.galois_key(gi))
    # element numbering: steps > 0 rotate left by 3^steps, < 0 by 3^(N/2 - |steps|), 0 = column swap
    for steps in (1, -1, 2, -4):
        assert o.galois_elt_from_step(steps) == M.galois_elt_from_step(steps, n)
    assert o.galois_elt_from_step(0) == 2 * n - 1
    cur = ct
    for step in M.naf(5):                                                     # 5 = 1 + 4: no direct key, two hops in this order
        e = M.galois_elt_from_step(step, n)
        nxt = o.apply_galois(cur, e)
        _check_galois(o, cur, nxt, e, o.galois_key(elts.index(e)))
        cur = nxt
    assert np.array_equal(cur, o.rotate_rows(ct, 5))
    cur = ct
    for step in M.naf(-7):                                                    # -7 = +1 - 8
        cur = o.apply_galois(cur, M.galois_elt_from_step(step, n))
    assert np.array_equal(cur, o.rotate_rows(ct, -7))
    assert M.naf(-7) == [1, -8] and M.naf(5) == [1, 4] and M.naf(3) == [-1, 4]
    _check_galois(o, ct, o.rotate_columns(ct), 2 * n - 1, o.galois_key(elts.index(2 * n - 1)))
    ext = _extreme_ct(o, "max")
    _check_galois(o, ext, o.apply_galois(ext, 3), 3, o.galois_key(elts.index(3)))
    if o.L.cno_batching(o.h):                                                 # the rotation rotates: slots move left by one inside both rows
        v = o.decode(o.decrypt(ct))
        r = o.decode(o.decrypt(o.rotate_rows(ct, 1)))
        assert np.array_equal(r[:n // 2], np.roll(v[:n // 2], -1)) and np.array_equal(r[n // 2:], np.roll(v[n // 2:], -1))


@XI
def test_key_material_has_the_documented_structure(xi):
    """the key layout the models read: key (l, d) = (-(a s + e) + 2^(dbc d) s' [only in limb l], a) at the evaluation points
    psi^(2 bitrev(p) + 1), psi the minimal primitive 2N-th root - K0 + K1 s - [j == l] 2^(dbc d) s^2 must be a SMALL polynomial (-e).
    xi-digits: the message term is (q/q_l) 2^(dbc d) s^2 in EVERY limb."""
    n, t, q, dbc = 64, 257, [0xffffee001, 0xffffc4001, 0x1ffffe0001], 10
    o = _oracle(n, t, q, dbc, 20, galois=False, xi=xi)
    Q = M.product(q)
    for j, qj in enumerate(q):
        assert o.psi(j) == M.minimal_primitive_root(n, qj)
    sk = [int(x) for x in o.secret_key()]
    rk = [int(x) for x in o.relin_key()]
    pos = 0
    for l in range(o.k):
        for d in range(-(-q[l].bit_length() // dbc)):
            for j, qj in enumerate(q):
                pts = M.eval_points(n, qj)
                s = sk[j * n:(j + 1) * n]
                k0 = rk[((pos * 2 + 0) * o.k + j) * n:][:n]
                k1 = rk[((pos * 2 + 1) * o.k + j) * n:][:n]
                msg = (Q // q[l]) * pow(2, dbc * d) % qj if xi else (pow(2, dbc * d, qj) if j == l else 0)
                vals = [(k0[p] + k1[p] * s[p] - msg * s[p] * s[p]) % qj for p in range(n)]
                # interpolate: the unique polynomial of degree < n with these values must have coefficients in [-19, 19] (clipped normal)
                # - checked by evaluating every candidate is impossible; instead invert the evaluation with the Vandermonde relation
                # e_i = n^-1 sum_p vals[p] x_p^-i  (x_p^n = -1: the points are the roots of x^n + 1)
                ninv = pow(n, -1, qj)
                for i in range(n):
                    c = sum(v * pow(x, -i, qj) for v, x in zip(vals, pts)) * ninv % qj
                    c = c - qj if c > qj // 2 else c
                    assert abs(c) <= 19
            pos += 1
    # the secret key itself is ternary in coefficient form
    pts = M.eval_points(n, q[0])
    s = sk[:n]
    ninv = pow(n, -1, q[0])
    coeffs = [sum(v * pow(x, -i, q[0]) for v, x in zip(s, pts)) * ninv % q[0] for i in range(n)]
    assert set(coeffs) <= {0, 1, q[0] - 1}


# ---------------------------------------------------------------------------------------------------- the tests above can fail
def test_the_two_key_switch_conventions_are_not_key_compatible():
    """what the start-up self-test of the drop-in exists for: keys of one convention under the digits of the other relinearize to words
    that differ from the client's AND no longer decrypt - rc 0 and garbage, unless somebody compares"""
    n, t, q, dbc = 64, 257, [0xffffee001, 0xffffc4001, 0x1ffffe0001], 10
    rng = np.random.default_rng(11)
    o = _oracle(n, t, q, dbc, 20, galois=False, xi=False)
    a, b = _fresh(o, rng), _fresh(o, rng)
    c3 = o.multiply(a, b)
    good = o.relinearize(c3)
    want = (o.decode(o.decrypt(a)).astype(object) * o.decode(o.decrypt(b)).astype(object)) % t
    assert [int(v) for v in o.decode(o.decrypt(good))] == [int(v) for v in want]
    o.set_ks_xi(True)                                       # same (raw-convention) keys, xi digits
    bad = o.relinearize(c3)
    assert not np.array_equal(good, bad)
    assert [int(v) for v in o.decode(o.decrypt(bad))] != [int(v) for v in want]
    o.set_ks_xi(False)
    assert np.array_equal(o.relinearize(c3), good)


@pytest.mark.parametrize("what", ["digit order high->low", "no plain lift", "beta dropped", "r not centred", "NAF high-order first", "upper-half increment dropped"])
def test_a_deviating_variant_is_caught(what, monkeypatch):
    """Mutation check: each free choice of SEAL 3.2 that still DECRYPTS correctly when made differently (digit order, plain lift, the
    floor's beta, the centring of r, the order of NAF hops, the upper-half increment) is changed in the MODEL - the word comparison with
    the oracle must then fail.  (If it did not, the assertions above would not be pinning that choice.)"""
    case = SMALL[0]
    if what == "digit order high->low":
        orig = M.digits_of
        monkeypatch.setattr(M, "digits_of", lambda limb, qj, dbc: orig(limb, qj, dbc)[::-1])
        run = lambda: test_relinearize_words(*case, False)
    elif what == "no plain lift":
        monkeypatch.setattr(M, "plain_lift", lambda m, qj, t: int(m))
        run = lambda: test_multiply_plain_words_full_size(Q8192[:2], 549764251649)
    elif what == "beta dropped":
        monkeypatch.setattr(M, "behz_floor", lambda d, q, t: (t * d) // M.product(q))
        run = lambda: test_multiply_words_equal_the_exact_integer_characterisation(*case)
    elif what == "r not centred":
        def lift(res, q):
            Q, X = M.product(q), 0
            for c, qj in zip(res, q):
                X += (int(c) * M.M_TILDE * pow(Q // qj, -1, qj) % qj) * (Q // qj)
            return (X + Q * ((-X * pow(Q, -1, M.M_TILDE)) % M.M_TILDE)) // M.M_TILDE
        monkeypatch.setattr(M, "behz_lift", lift)
        run = lambda: test_multiply_words_equal_the_exact_integer_characterisation(*case)
    elif what == "NAF high-order first":
        orig = M.naf
        monkeypatch.setattr(M, "naf", lambda v: orig(v)[::-1])
        run = lambda: test_apply_galois_and_rotation_words(*case, False)
    else:
        orig = M.add_plain
        def no_increment(ct, plain, q, t, subtract=False):
            Q = M.product(q)
            out = [[list(l) for l in p] for p in ct]
            for j, qj in enumerate(q):
                for i, m in enumerate(plain):
                    s = (Q // t) * int(m) % qj
                    out[0][j][i] = (out[0][j][i] - s) % qj if subtract else (out[0][j][i] + s) % qj
            return out
        monkeypatch.setattr(M, "add_plain", no_increment)
        run = lambda: test_add_plain_words_full_size(Q8192[:2], 549764251649)
    with pytest.raises(AssertionError):
        run()
