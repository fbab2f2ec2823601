"""GPU: cn_noise_norm - exact norms of planted noise polynomials (no key in the result: c1 = c2 = 0, c0 = [X t^-1]_q), norms of real
ciphertexts against the host composition of cn_noise_poly's words, the budgets derived from them, the call's errors, the flush of deferred
work, and levels.min_budget against the per-ciphertext budgets."""
import math
import random

import numpy as np
import pytest

from conftest import PARAMS
from noise_norm_model import centred, prod

pytestmark = pytest.mark.gpu

C3 = [0x7fffffd8001, 0x7fffffc8001, 0xfffffffc001, 0xffffff6c001, 0xfffffebc001]        # = COEFF_MODULUS_128[8192]
C9 = list(PARAMS["c5"]["q"]) + [0x1ffffffe48001]                                       # = COEFF_MODULUS_128[16384]
CHAINS = {"c3": (8192, PARAMS["c3"]["t"], C3), "c9": (16384, PARAMS["c5"]["t"], C9),
          "c12": (8192, PARAMS["c3"]["t"], C3 + C9[:7])}                               # 12 limbs: every prime is 1 mod 16384
PASS_WORDS = 1 << 24            # cn_noise_norm: at most max(1, 2^24 / (k N)) ciphertexts per pass (include/cnhip.h)


def keyed(chain, galois=False):
    from cryptonets_amd._native import Context
    n, t, q = CHAINS[chain]
    g = Context(n, t, q=list(q), dbc=60 if n == 16384 else 10, gdbc=60 if n == 16384 else 20, device=0)
    g.keygen(77, galois=galois)
    return g


def every_level(g):
    return [g.level(l) for l in range(1, g.k)] + [g]


def host_norms(g, h, ci, count):
    """the old probe: cn_noise_poly's words composed with Python integers"""
    w = g.noise_poly(h, ci, count)
    Q = prod(g.q)
    coef = [(Q // m) * pow((Q // m) % m, -1, m) for m in g.q]
    out = []
    for c in range(count):
        x = sum(w[c, j].astype(object) * coef[j] for j in range(g.k)) % Q
        out.append(max(centred(int(v), Q) for v in x))
    return out


def planted(g, cts, size=2):
    """ciphertexts whose noise polynomial t (c0 + c1 s + c2 s^2) mod q is exactly the given {coefficient: X} (c1 = c2 = 0)"""
    Q, n, k = prod(g.q), g.n, g.k
    tinv = pow(g.t, -1, Q)
    words = np.zeros((len(cts), size * k * n), dtype=np.uint64)
    for c, vals in enumerate(cts):
        for pos, X in vals.items():
            c0 = X * tinv % Q
            for j, m in enumerate(g.q):
                words[c, j * n + pos] = c0 % m
    h = g.ct_alloc(len(cts), size)
    g.ct_upload(h, 0, words)
    return h, [max([centred(X % Q, Q) for X in vals.values()] + [0]) for vals in cts]


def edge_values(Q):
    out = [0, 1, Q - 1, (Q - 1) // 2, (Q + 1) // 2]
    for b in range(64, Q.bit_length(), 64):
        out += [(1 << b) - 1, 1 << b]
    return out


def check_exact(g, rng, size):
    Q, n = prod(g.q), g.n
    # every edge value, its maximum at coefficient 0, N - 1 or a random one, beside a smaller decoy of the other sign
    cts = []
    for i, X in enumerate(edge_values(Q)):
        pos = [0, n - 1, int(rng.integers(1, n - 1))][i % 3]
        m = centred(X, Q) // 3
        cts.append({pos: X, (pos + 1 + int(rng.integers(0, n - 2))) % n: m if i % 2 else (Q - m) % Q})
    h, exp = planted(g, cts, size)
    assert g.noise_norm(h, 0, len(cts)) == exp, (g.k, size)
    g.free(h)
    # a batch of distinct norms with the largest first, in the middle, last
    rnd = random.Random(int(rng.integers(0, 1 << 30)))
    norms = set()
    while len(norms) < 7:
        norms.add(rnd.randrange(1, Q // 2))
    norms = sorted(norms)
    for top in (0, 3, 6):
        order = norms[:-1]
        order.insert(top, norms[-1])
        cts = [{int(rng.integers(0, n)): (v if c % 2 else Q - v)} for c, v in enumerate(order)]
        h, exp = planted(g, cts, size)
        got = g.noise_norm(h, 0, 7)
        assert got == exp and got[top] == max(got), (g.k, size, top)
        assert g.noise_norm(h, 2, 4) == exp[2:6]
        g.free(h)


@pytest.mark.parametrize("chain", ["c3", "c9", "c12"])
def test_planted_norms_are_exact_at_every_level(chain, rng):
    g = keyed(chain)
    for lv in every_level(g):
        check_exact(lv, rng, 2)
    check_exact(g, rng, 3)


@pytest.mark.parametrize("chain", ["c3", "c9", "c12"])
def test_counts_across_passes(chain, rng):
    g = keyed(chain)
    for lv in every_level(g):
        Q, n = prod(lv.q), lv.n
        per = max(1, PASS_WORDS // (lv.k * n))
        count = per + 2
        marks = {1: Q - 5, per - 1: 1 << 40, per: (Q - 1) // 2, per + 1: 7, count: Q - (1 << 50)}        # the first probed, both sides of the cut, the last
        cts = [{int(rng.integers(0, n)): marks[c]} if c in marks else {} for c in range(count + 1)]
        h, exp = planted(lv, cts)
        assert lv.noise_norm(h, 1, count) == exp[1:], lv.k
        lv.free(h)


# ------------------------------------------------------------------ real ciphertexts
def budgets_from(norms, q):
    Q = prod(q)
    return ([max(0, Q.bit_length() - v.bit_length() - 1) for v in norms],
            [math.log2(Q) - (math.log2(v) if v else 0.0) - 1.0 for v in norms])


def check_real(g, h, count):
    norms = g.noise_norm(h, 0, count)
    assert norms == host_norms(g, h, 0, count)
    ints, floats = budgets_from(norms, g.q)
    assert g.invariant_noise_budget(h, 0, count, exact_bits=True) == ints
    assert g.invariant_noise_budget(h, 0, count) == floats
    return norms


def fresh(g, rng, count):
    pt = g.pt_alloc(count)
    g.encode_batch(rng.integers(0, g.t, size=(count, g.n), dtype=np.uint64), pt, 0)
    h = g.ct_alloc(count)
    g.encrypt(pt, 0, h, 0, count, seed=5)
    g.free(pt)
    return h


@pytest.mark.parametrize("chain,galois", [("c3", True), ("c9", False)])
def test_real_ciphertexts_match_the_host_composition(chain, galois, rng):
    g = keyed(chain, galois=galois)
    count = 6
    a, b = fresh(g, rng, count), fresh(g, rng, count)
    na = check_real(g, a, count)
    prod2 = g.ct_alloc(count)
    g.mul_relin(a, 0, b, 0, prod2, 0, count)
    nm = check_real(g, prod2, count)
    assert min(nm) > max(na)
    prod3 = g.ct_alloc(count, 3)
    g.multiply(a, 0, b, 0, prod3, 0, count)
    check_real(g, prod3, count)
    if galois:
        rot = g.ct_alloc(count)
        g.rotate_rows(prod2, 0, 1, rot, 0, count)
        check_real(g, rot, count)
    for limbs in (g.k - 1, 2, 1):
        lv = g.level(limbs)
        for src, size in ((prod2, 2), (prod3, 3)):
            out = lv.ct_alloc(count, size)
            g.mod_switch(src, 0, count, lv, out, 0)
            check_real(lv, out, count)
            lv.free(out)


@pytest.mark.parametrize("name", ["c2", "c4"])
def test_oracle_ciphertexts_match_the_oracle_budget(name, rng):
    from cryptonets_amd._native import Context
    from oracle.cno import Oracle
    from oracle_backend import OracleClient
    p = PARAMS[name]
    g = Context(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)
    g.keygen(123, galois=False)
    o = Oracle(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"])
    o.import_keys(g.get_key(3), g.get_key(2))
    oc = OracleClient(p["t"], p["n"], p["q"], p["dbc"], p["gdbc"], oracle=o)
    a = o.encrypt(o.encode(rng.integers(0, p["t"], size=p["n"], dtype=np.uint64)))
    b = o.encrypt(o.encode(rng.integers(0, p["t"], size=p["n"], dtype=np.uint64)))
    c3 = o.multiply(a, b)
    h2, h3 = g.ct_alloc(2, 2), g.ct_alloc(1, 3)
    g.ct_upload(h2, 0, np.stack([a, b]))
    g.ct_upload(h3, 0, c3[None, :])
    assert g.invariant_noise_budget(h2, 0, 2, exact_bits=True) == [oc.noise_budget_words(a), oc.noise_budget_words(b)]
    assert g.invariant_noise_budget(h3, 0, 1, exact_bits=True) == [oc.noise_budget_words(c3)]


# ------------------------------------------------------------------ call behaviour
def test_errors_graph_refusal_and_empty_calls():
    from cryptonets_amd._native import CnError, Context, _p64
    n, t, q = CHAINS["c3"]
    bare = Context(n, t, q=list(q), device=0)
    h = bare.ct_alloc(2)
    with pytest.raises(CnError) as e:
        bare.noise_norm(h, 0, 1)
    assert e.value.code == -3                                          # CN_ERR_NOKEY
    bare.free(h)
    g = keyed("c3")
    h = g.ct_alloc(3)
    for ci, count in ((3, 1), (2, 2), (0, 4)):
        with pytest.raises(CnError) as e:
            g.noise_norm(h, ci, count)
        assert e.value.code == -1, (ci, count)                         # CN_ERR_ARG
    assert g.L.cn_noise_norm(g._h, h, 0, 1, None) == -1                # null host
    buf = np.full(4, 99, dtype=np.uint64)
    assert g.L.cn_noise_norm(g._h, h, 3, 0, _p64(buf)) == 0 and (buf == 99).all()     # count 0: nothing written
    assert g.noise_norm(h, 0, 0) == []
    g.graph_begin()
    try:
        g.add(h, 0, h, 1, h, 1)
        with pytest.raises(CnError) as e:
            g.noise_norm(h, 0, 1)
        assert e.value.code == -1
    finally:
        graph = g.graph_end()
    g.free(graph)
    assert g.noise_norm(h, 0, 3) == [0, 0, 0]                          # zero words: the zero polynomial
    g.free(h)


def test_deferred_mul_relin_is_flushed_before_the_probe(rng):
    g = keyed("c3")
    a, b = fresh(g, rng, 1), fresh(g, rng, 1)
    out, ref = g.ct_alloc(1), g.ct_alloc(1)
    g.copy(a, 0, out, 0, 1)                                            # a stale probe would see a's fresh noise
    stale = g.noise_norm(out, 0, 1)
    g.set_option("defer", 1)
    try:
        g.mul_relin(a, 0, b, 0, out, 0, 1)
        assert g.get_option("pending_calls") == 1                      # queued, not run
        queued = g.invariant_noise_budget(out, 0, 1, exact_bits=True)
        assert g.get_option("pending_calls") == 0
    finally:
        g.set_option("defer", 0)
    g.mul_relin(a, 0, b, 0, ref, 0, 1)
    g.sync()
    assert queued == g.invariant_noise_budget(ref, 0, 1, exact_bits=True)
    assert g.noise_norm(out, 0, 1) == g.noise_norm(ref, 0, 1) != stale


# ------------------------------------------------------------------ levels.min_budget
def test_min_budget_equals_the_minimum_of_the_per_ciphertext_budgets():
    """a CryptoNets-shaped matrix (845 columns, one ciphertext each, both plaintext primes) after a multiply"""
    from cryptonets_amd.cryptonets_mnist import PLAIN_PRIMES
    from cryptonets_amd.hewrapper import EMatrixFormat, EncryptedSealBfvFactory
    from cryptonets_amd.levels import min_budget
    Factory = EncryptedSealBfvFactory(list(PLAIN_PRIMES), 8192, client_seed=1234)
    env = Factory.AllocateComputationEnv()
    rng = np.random.default_rng(3)
    m = Factory.GetEncryptedMatrix(rng.integers(-4, 5, size=(8192, 845)).astype(np.float64), EMatrixFormat.ColumnMajor, 1)
    sq = m.ElementWiseMultiply(m, env)
    per = []
    for col in sq.leVectors:
        for atom, e in zip(col.eVectors, env.Environments):
            d = atom.encData
            per += e.client.noise_budget(d.h, d.first, d.count)
    assert min_budget([sq], Factory) == float(min(per))
