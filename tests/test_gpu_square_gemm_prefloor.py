"""cn_square_gemm with ONE fast floor per dense output for components 0 and 1 ("sg_prefloor") against the CPU oracle and the form that floors every product.

The form sums the Bsk words of d0 and d1 in NTT form (k_scalar_gemm_mfma<.., GemmBskForm>: seven signed byte digits, mod b), the canonical y of their q words as exact
64-bit integers (<.., GemmYForm>), transforms the Bsk sums back once per output and runs the floor tail per output (k_behz_floor_out).  It must write the words of the old
form.  Every case runs the same plan under "sg_prefloor" = 2 (the new form for any K) and = 0, compares both word for word with the oracle's mul_relin_batch +
scalar_gemm + add_plain_batch, and reads "square_gemm_prefloor" back.

Shapes: N = 1024 with three limbs ("tiny") and N = 4096 with two (tiny's first two moduli: both are 1 mod 8192); K = 1, 3 (one partial K step), 33 (two steps), 65 (a
full turn of the kernel's three-set ring: it crosses a 32-wide step twice); M = 16 (half an output tile) and 33 (two tiles, one row in the second).  Inputs: those of
test_square_gemm.inputs (q - 1 everywhere, zero, q / 2 in c0, then uniform).  Weights: signed, one row of the largest weight, one alternating in sign, a zero weight in
every row but the first two, and - "a zero row" - one output whose only non-zero weight sits on the all-zero input (the planner refuses a row without any term, as
AddMany of nothing is an error in the reference); a bias per output.  The oracle squares the 65 inputs of a ring once.
"""
import numpy as np
import pytest

from conftest import PARAMS
from test_square_gemm import fresh_context, inputs, res, small_weights

pytestmark = pytest.mark.gpu

RINGS = {"n1024k3": dict(PARAMS["tiny"]), "n4096k2": dict(n=4096, t=40961, q=PARAMS["tiny"]["q"][:2], dbc=10, gdbc=20)}
_rings, _squares = {}, {}


def ring(name):
    """(oracle, its 65 inputs, their relinearized squares): once per ring"""
    from oracle.cno import Oracle
    if name not in _rings:
        p = RINGS[name]
        o = Oracle(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"])
        o.keygen(11, galois=False)
        X = inputs(o, 65, 0x9F1 + p["n"])
        X.setflags(write=False)
        sq = o.mul_relin_batch(X, X)
        sq.setflags(write=False)
        _rings[name] = (o, X, sq)
    return _rings[name]


def context(name, o):
    from cryptonets_amd._native import Context
    p = RINGS[name]
    g = Context(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)
    g.set_relin_key(o.relin_key())
    return g


def weights(rng, O, K, t, wmax):
    W = small_weights(rng, O, K, t, wmax)
    W[0, :] = wmax
    if O > 1:
        W[1, ::2] = -wmax
    for r in range(2, O):
        if K > 1:
            W[r, (r * 7) % K] = 0
    if K >= 2 and O > 2:
        W[2, :] = 0
        W[2, 1] = 5                                                  # input 1 is the all-zero ciphertext: the products of this row are all zero
    return W


def run_two_forms(g, X, W, O, bias):
    """words and counter steps of the same plan under sg_prefloor = 2 and = 0"""
    h, a, b, bh = g.ct_alloc(len(X)), g.ct_alloc(O + 1), g.ct_alloc(O + 1), g.pt_alloc(O)
    g.ct_upload(h, 0, X)
    g.pt_upload(bh, 0, bias)
    plan = g.gemm_plan(W, bias_pt=bh, bias_idx=np.arange(O, dtype=np.int32))
    out = []
    for mode, dst in ((2, a), (0, b)):
        g.set_option("sg_prefloor", mode)
        p0, f0 = g.get_option("square_gemm_prefloor"), g.get_option("square_gemm_fused")
        g.square_gemm(plan, h, 0, dst, 1)
        out.append((g.ct_download(dst, 1, O), g.get_option("square_gemm_prefloor") - p0, g.get_option("square_gemm_fused") - f0))
    g.set_option("sg_prefloor", 1)
    for x in (h, a, b, bh, plan):
        g.free(x)
    return out


def biases(o, O, t):
    return np.stack([o.encode(np.full(o.n, (v * 977 + 1) % t, dtype=np.uint64)) for v in range(O)])


@pytest.mark.parametrize("O", [16, 33])
@pytest.mark.parametrize("K", [1, 3, 33, 65])
@pytest.mark.parametrize("name", ["n1024k3", "n4096k2"])
def test_words_of_the_oracle_and_of_the_old_form(name, K, O):
    o, X, sq = ring(name)
    g = context(name, o)
    try:
        t = RINGS[name]["t"]
        W = weights(np.random.default_rng(0xF100 + 64 * K + O), O, K, t, t // 2)
        bias = biases(o, O, t)
        want = o.add_plain_batch(o.scalar_gemm(sq[:K], res(W, t)), bias)
        (new, p_new, f_new), (old, p_old, f_old) = run_two_forms(g, X[:K], res(W, t), O, bias)
        assert (p_new, f_new) == (1, 1), "sg_prefloor = 2 runs the new form and still counts as a fused call"
        assert (p_old, f_old) == (0, 1)
        assert np.array_equal(old, want)
        assert np.array_equal(new, want)
    finally:
        g.close()


def test_default_gate_keeps_small_layers_and_narrow_layers_on_the_old_form():
    """under the default (1) a layer below SG_PREFLOOR_MIN_K terms floors every product, as every launch-count test expects; fewer than 16 outputs never take the
    matrix cores, so M = 10 counts 0 even under sg_prefloor = 2"""
    name = "n1024k3"
    o, X, sq = ring(name)
    g = context(name, o)
    try:
        t, K = RINGS[name]["t"], 65
        assert g.get_option("sg_prefloor") in (0, 1) and K < g.get_option("sg_prefloor_min_k")
        for O, mode, step in ((16, g.get_option("sg_prefloor"), 0), (10, 2, 0), (16, 2, 1)):
            W = res(weights(np.random.default_rng(0xD0 + O), O, K, t, 100), t)
            bias = biases(o, O, t)
            h, a, bh = g.ct_alloc(K), g.ct_alloc(O), g.pt_alloc(O)
            g.ct_upload(h, 0, X[:K])
            g.pt_upload(bh, 0, bias)
            plan = g.gemm_plan(W, bias_pt=bh, bias_idx=np.arange(O, dtype=np.int32))
            g.set_option("sg_prefloor", mode)
            p0 = g.get_option("square_gemm_prefloor")
            g.square_gemm(plan, h, 0, a, 0)
            assert g.get_option("square_gemm_prefloor") - p0 == step, (O, mode)
            assert np.array_equal(g.ct_download(a, 0, O), o.add_plain_batch(o.scalar_gemm(sq[:K], W), bias))
            for x in (h, a, bh, plan):
                g.free(x)
    finally:
        g.close()


def test_plan_whose_bound_fails_runs_the_old_form():
    """CryptoNets ring, 8 weights of 2^20 - 1 per row: 8 R t N q = 2^(3 + 23 + 39 + 13 + 218) = 2^296 passes B m_sk / 2 < 2^293 - the gate says no even
    under sg_prefloor = 2, and the words are those of the oracle"""
    o, g = fresh_context("c3")
    try:
        t, K, O = PARAMS["c3"]["t"], 8, 16
        W = small_weights(np.random.default_rng(0xB0), O, K, t, (1 << 20) - 1)
        W[0, :] = (1 << 20) - 1
        X = inputs(o, K, 0xB0B)
        bias = biases(o, O, t)
        (new, p_new, f_new), (old, p_old, f_old) = run_two_forms(g, X, res(W, t), O, bias)
        assert (p_new, f_new, p_old, f_old) == (0, 1, 0, 1)
        assert np.array_equal(new, old)
        assert np.array_equal(new, o.add_plain_batch(o.scalar_gemm(o.mul_relin_batch(X, X), res(W, t)), bias))
    finally:
        g.close()


def test_cryptonets_ring():
    """N = 8192, five limbs of 44 bits, six 49-bit auxiliary primes (seven byte digits), K = 40 (two K steps), M = 16; |w| <= 1000: R <= 40000, inside the bound"""
    o, g = fresh_context("c3")
    try:
        t, K, O = PARAMS["c3"]["t"], 40, 16
        W = weights(np.random.default_rng(0xC3F), O, K, t, 1000)
        X = inputs(o, K, 0xC3F1)
        bias = biases(o, O, t)
        (new, p_new, f_new), (old, p_old, f_old) = run_two_forms(g, X, res(W, t), O, bias)
        assert (p_new, f_new, p_old, f_old) == (1, 1, 0, 1)
        assert np.array_equal(new, old)
        assert np.array_equal(new, o.add_plain_batch(o.scalar_gemm(o.mul_relin_batch(X, X), res(W, t)), bias))
    finally:
        g.close()
