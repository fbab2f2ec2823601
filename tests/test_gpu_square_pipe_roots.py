"""k_square_pipe with every root of its transforms resident: word for word against the CPU oracle and against k_square_fused.

The kernel stages indices [0, N/2) of the forward and of the inverse root table behind its exchange image, keeps a thread's eight last-pass roots of each direction in
registers, and requests the next operand a step ahead.  What that can get wrong and the shape that shows it:
  the half tables and the register roots, per ring size and policy   N = 1024, 2048, 4096 on the first two moduli of the sets of tests/size_policy_sets.py - a
                                                                     44 / 40-bit pair (ArF64L) and a 49 / 49-bit pair (ArF64: the forward recentring) - and
                                                                     N = 8192 on the CryptoNets ring (five limbs)
  the request-ahead and the last block of a workgroup, which         two q limbs and three Bsk limbs on 256 CUs make 128 and 85 resident workgroups per modulus:
  re-reads its own operand and drops it                              1, 130 and 300 products give them 1, 1 - 2 and 2 - 4 blocks, unevenly; 60 products on five
                                                                     and six limbs (51 and 42 workgroups) 1 - 2
  the NttOut01 form (d0, d1 leave in NTT form, no inverse            cn_square_gemm under "sg_prefloor" = 2 with 16 outputs and K = 130 on the smallest ring that
  transform between step 0 and step 1)                               form accepts (N = 1024, three limbs), against "sg_prefloor" = 0
Every squaring runs under "sq_pipe" = 2 (k_square_pipe for any count) and = 0 (k_square_fused); the three word arrays must be equal.  Outputs lie between two
sentinel ciphertexts that must keep their words.  The oracle squares the inputs of a ring once, for the largest count; the cases slice it.
"""
import numpy as np
import pytest

from conftest import PARAMS, get_oracle
from size_policy_sets import Q, T, edge_words, uniform
from test_gpu_square_gemm_prefloor import biases, run_two_forms, weights
from test_square_gemm import inputs, res

pytestmark = pytest.mark.gpu

PAIRS = {"f64l": Q["f64l"][:2], "f64": Q["f64"][:2]}
assert [m.bit_length() for m in PAIRS["f64l"]] == [44, 40] and [m.bit_length() for m in PAIRS["f64"]] == [49, 49]
COUNTS = {1024: (1, 130, 300), 2048: (130,), 4096: (130,)}
_rings = {}


def ring(policy, n):
    """(oracle, inputs, their relinearized squares) of a two-limb ring: once per (policy, N), for the largest count of the ring"""
    from oracle.cno import Oracle
    if (policy, n) not in _rings:
        o = Oracle(n, T, q=PAIRS[policy], dbc=60, gdbc=60)
        o.keygen(29, galois=False)
        X = edge_words(o, np.random.default_rng(0x5A0 + n), max(COUNTS[n]))
        sq = o.mul_relin_batch(X, X)
        for a in (X, sq):
            a.setflags(write=False)
        _rings[(policy, n)] = (o, X, sq)
    return _rings[(policy, n)]


def squares_on_both_kernels(g, o, X):
    """the words of cn_mul_relin(X, X) under "sq_pipe" = 2 and = 0, each between two sentinels, and the launches of each call"""
    count = len(X)
    h, out = g.ct_alloc(count + 1), g.ct_alloc(count + 2)
    g.ct_upload(h, 1, X)
    sentinel = uniform(o, np.random.default_rng(count), count + 2)
    got = {}
    for mode in (2, 0, -1):                                           # -1: the separate transforms ("sq_fused" = 0)
        g.set_option("sq_pipe", max(mode, 0))
        g.set_option("sq_fused", 0 if mode < 0 else 1)
        g.ct_upload(out, 0, sentinel)
        s0 = g.stats()["kernel_launches"]
        g.mul_relin(h, 1, h, 1, out, 1, count)
        words = g.ct_download(out, 0, count + 2)
        assert np.array_equal(words[0], sentinel[0]) and np.array_equal(words[-1], sentinel[-1]), "a ciphertext beside the written range changed"
        got[mode] = (words[1:-1], g.stats()["kernel_launches"] - s0)
    assert np.array_equal(g.ct_download(h, 1, count), X), "the operands changed"
    g.set_option("sq_pipe", 1)
    g.set_option("sq_fused", 1)
    for x in (h, out):
        g.free(x)
    return got


def check(g, o, X, want):
    got = squares_on_both_kernels(g, o, X)
    (pipe, l_pipe), (fused, l_fused), (separate, l_separate) = got[2], got[0], got[-1]
    # one squaring kernel per base instead of transforms + k_intt_tensor (as tests/test_gpu_size_policy_matrix.py counts them): a fused kernel did run
    assert l_pipe == l_fused == l_separate - 2, (l_pipe, l_fused, l_separate)
    assert np.array_equal(separate, want)
    assert np.array_equal(fused, want)
    bad = np.flatnonzero((pipe != want).any(axis=1))
    assert bad.size == 0, "products that differ from the oracle: %s" % bad[:16]


@pytest.mark.parametrize("n,count", [(n, c) for n in COUNTS for c in COUNTS[n]])
@pytest.mark.parametrize("policy", ["f64l", "f64"])
def test_squarings_on_two_limbs(policy, n, count):
    from cryptonets_amd._native import Context
    o, X, sq = ring(policy, n)
    g = Context(n, T, q=PAIRS[policy], dbc=60, gdbc=60, device=0)
    try:
        g.set_relin_key(o.relin_key())
        check(g, o, X[:count], sq[:count])
    finally:
        g.close()


def test_cryptonets_ring_60_products():
    """N = 8192, five q limbs and six Bsk limbs: 51 and 42 resident workgroups per modulus, so 9 and 18 of them square two blocks"""
    from cryptonets_amd._native import Context
    p = PARAMS["c3"]
    o = get_oracle("c3", galois=False)
    g = Context(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)
    try:
        g.set_relin_key(o.relin_key())
        X = inputs(o, 60, 0x5A13)
        check(g, o, X, o.mul_relin_batch(X, X))
    finally:
        g.close()


def test_ntt_form_outputs_through_square_gemm():
    """k_square_pipe<.., NttOut01> on the Bsk side: 16 outputs of K = 130 squares.  Weights up to 3000: the row of the largest weight sums to 390 000, below the
    399 360 that tests/test_gpu_square_gemm_prefloor.py runs on this ring (K = 65 at t / 2), so the bound of the form holds and "square_gemm_prefloor" must count."""
    from cryptonets_amd._native import Context
    from oracle.cno import Oracle
    p = PARAMS["tiny"]
    o = Oracle(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"])
    o.keygen(11, galois=False)
    K, O, t = 130, 16, p["t"]
    X = inputs(o, K, 0x5A17)
    W = res(weights(np.random.default_rng(0x5A18), O, K, t, 3000), t)
    bias = biases(o, O, t)
    want = o.add_plain_batch(o.scalar_gemm(o.mul_relin_batch(X, X), W), bias)
    g = Context(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)
    try:
        g.set_relin_key(o.relin_key())
        g.set_option("sq_pipe", 2)
        (new, p_new, f_new), (old, p_old, f_old) = run_two_forms(g, X, W, O, bias)
        assert (p_new, f_new, p_old, f_old) == (1, 1, 0, 1)
        assert np.array_equal(old, want)
        assert np.array_equal(new, want)
    finally:
        g.close()
