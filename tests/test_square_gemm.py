"""cn_square_gemm - SquareActivation and the dense layer behind it in one call - against its two separate steps and the CPU oracle.

The call must write the words of cn_mul_relin followed by cn_gemm_plan_apply (tests/test_square_gemm_identity.py: why one key switch per
dense OUTPUT, fed with weight-combined digit polynomials, gives them).  Every case is compared word for word with the oracle's
mul_relin_batch + scalar_gemm + add_plain_batch and with the library's own two calls; "square_gemm_fused" reads back which form ran.

Shapes: the smallest register-radix ring ("tiny": N = 1024, three limbs, dbc 10) with 3 and 7 inputs -> 2 outputs (two-launch key switch
with a workgroup per digit, two-output tile of the digit GEMM) and 40 -> 16 (a workgroup per source limb, two ten-output tiles, the second
partly empty); the CryptoNets ring ("c3": N = 8192, five limbs) with 8 -> 40 (200 (ciphertext, limb) workgroups: the fused key-switch kernel)
and 8 -> 2.  The digit GEMM has one form, FP64 with one FMA per term: the 40 -> 16 case runs it where the plain GEMM takes the matrix cores.
"""
import numpy as np
import pytest

from conftest import PARAMS, get_oracle

pytestmark = pytest.mark.gpu

COUNTERS = ("Multiplication", "Relinarization", "PlainMultiplication", "Addition", "PlainAddition")


def res(w, t):
    return np.mod(np.asarray(w, dtype=np.int64), t).astype(np.uint64)


def fresh_context(name, xi=False):
    from cryptonets_amd._native import Context
    p = PARAMS[name]
    if xi:
        from oracle.cno import Oracle
        o = Oracle(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], ks_xi=True)
        o.keygen(11, galois=False)
    else:
        o = get_oracle(name, galois=False)
    g = Context(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)
    if xi:
        g.set_option("ks_xi", 1)
    g.set_relin_key(o.relin_key())
    return o, g


def inputs(o, count, seed):
    """uniform ciphertext words; the first three with residues at the edges of the range (q - 1, 0, q / 2 in c0)"""
    from bench import uniform_ct_words
    X = uniform_ct_words(np.random.default_rng(seed), o.q, o.n, count)
    w = X[:min(3, count)].reshape(-1, 2, o.k, o.n)
    for j, qj in enumerate(o.q):
        w[0, :, j, :] = qj - 1
        if len(w) > 1:
            w[1, :, j, :] = 0
        if len(w) > 2:
            w[2, 0, j, :] = qj // 2
    return X


def expected(o, X, W, idx=None, bias=None):
    sq = o.mul_relin_batch(X, X)
    out = o.scalar_gemm(sq, W, idx)
    return o.add_plain_batch(out, bias) if bias is not None else out


def run_both(g, X, W, O, idx=None, bias=None, out_extra=0):
    """(cn_square_gemm words, cn_mul_relin + cn_gemm_plan_apply words, fused calls counted)"""
    h, sq, a, b = g.ct_alloc(len(X)), g.ct_alloc(len(X)), g.ct_alloc(O + out_extra), g.ct_alloc(O)
    g.ct_upload(h, 0, X)
    bh = 0
    if bias is not None:
        bh = g.pt_alloc(len(bias))
        g.pt_upload(bh, 0, bias)
    plan = g.gemm_plan(W, idx=idx, bias_pt=bh, bias_idx=np.arange(O, dtype=np.int32) if bias is not None else None)
    before = g.get_option("square_gemm_fused")
    g.square_gemm(plan, h, 0, a, out_extra)
    fused = g.get_option("square_gemm_fused") - before
    g.mul_relin(h, 0, h, 0, sq, 0, len(X))
    g.gemm_apply(plan, sq, b, 0)
    return g.ct_download(a, out_extra, O), g.ct_download(b, 0, O), fused


def small_weights(rng, O, K, t, wmax):
    W = rng.integers(-wmax, wmax + 1, size=(O, K))
    W[W == 0] = 1
    return W


@pytest.mark.parametrize("name,K,O", [("tiny", 3, 2), ("tiny", 7, 2), ("tiny", 40, 16), ("c3", 8, 40), ("c3", 8, 2)])
def test_square_gemm_gives_the_words_of_its_two_steps(name, K, O):
    o, g = fresh_context(name)
    try:
        t = PARAMS[name]["t"]
        rng = np.random.default_rng(0x5147 + K + O)
        # row sums below min q / 2 / (2^dbc - 1): tiny's 36-bit moduli leave sum |w| < 2^25, so the 40-term rows stay below 2^19 per weight
        wmax = (1 << 20) - 1 if name == "c3" or K <= 7 else (1 << 19) - 1
        W = small_weights(rng, O, K, t, wmax)
        W[0, :] = wmax                                               # the largest row sum
        W[1, ::2] = -wmax
        X = inputs(o, K, 0x51 + K)
        got, two, fused = run_both(g, X, res(W, t), O)
        assert fused == 1, "the case is meant to run one key switch per output"
        assert np.array_equal(got, two)
        assert np.array_equal(got, expected(o, X, res(W, t)))
    finally:
        g.close()


def test_gather_lists_zero_weights_and_bias():
    """two gather lists with padded taps (-1) and zero weights, a bias per output, the outputs at an offset of their handle"""
    name, K, O = "tiny", 6, 5
    o, g = fresh_context(name)
    try:
        t = PARAMS[name]["t"]
        rng = np.random.default_rng(0x6A7)
        idx = np.array([[0, 1, 2, -1, 4, 5]] * 3 + [[6, 5, -1, 3, 2, -1]] * 2, dtype=np.int32)
        W = small_weights(rng, O, K, t, 1000)
        W[0, 1] = 0
        W[3, 0] = 0
        W[4, 5] = 77                                                 # a weight on a padded tap counts for nothing
        X = inputs(o, 7, 0x77)
        bias = np.stack([o.encode(np.full(o.n, v, dtype=np.uint64)) for v in (1, 2, t - 3, 4, 5)])
        got, two, fused = run_both(g, X, res(W, t), O, idx=idx, bias=bias, out_extra=2)
        assert fused == 1
        assert np.array_equal(got, two)
        assert np.array_equal(got, expected(o, X, res(W, t), idx=idx, bias=bias))
    finally:
        g.close()


@pytest.mark.parametrize("why", ["row_sum_above_the_bound", "ks_xi"])
def test_ineligible_calls_take_the_two_steps_and_still_agree(why):
    """tiny's 36-bit moduli bound a row at sum |w| < 2^25: 40 weights up to t / 2 = 6144 fit, so the bound is crossed by repeating the inputs in a row of 8000
    terms; "ks_xi" = 1 (digits of [c_l (q/q_l)^-1]) has no digit GEMM"""
    name, O = "tiny", 3
    o, g = fresh_context(name, xi=why == "ks_xi")
    try:
        t = PARAMS[name]["t"]
        rng = np.random.default_rng(0xFA11)
        K, idx = 40, None
        if why == "row_sum_above_the_bound":
            K = 8000
            idx = np.tile(np.arange(40, dtype=np.int32), (O, K // 40))
            W = np.full((O, K), (t - 1) // 2, dtype=np.int64)
            assert K * ((t - 1) // 2) * 1023 >= min(o.q) // 2
        else:
            W = small_weights(rng, O, K, t, 100)
        X = inputs(o, 40, 0xFA)
        got, two, fused = run_both(g, X, res(W, t), O, idx=idx)
        assert fused == 0
        assert np.array_equal(got, two)
        assert np.array_equal(got, expected(o, X, res(W, t), idx=idx))
    finally:
        g.close()


def test_weights_beyond_2_20_and_row_sums_beyond_the_bound_fall_back_at_c3():
    """c3's t has 40 bits: a weight of 2^20 is not "small" any more; and its 43-bit moduli bound a row at sum |w| (2^10 - 1) < 2^42, crossed here by a row of
    4200 terms (repeated inputs) of weight 2^20 - 1"""
    name = "c3"
    o, g = fresh_context(name)
    try:
        t = PARAMS[name]["t"]
        X = inputs(o, 4, 0xC3)
        big = np.array([[1 << 20, 3, t - 5, 7], [2, (1 << 20) + 1, 1, 1]], dtype=np.uint64)
        got, two, fused = run_both(g, X, big, 2)
        assert fused == 0
        assert np.array_equal(got, two)
        assert np.array_equal(got, expected(o, X, big))
        K = 4200
        idx = np.tile(np.arange(4, dtype=np.int32), (2, K // 4))
        W = np.full((2, K), (1 << 20) - 1, dtype=np.uint64)
        assert K * ((1 << 20) - 1) * 1023 >= min(o.q) // 2
        got, two, fused = run_both(g, X, W, 2, idx=idx)
        assert fused == 0
        assert np.array_equal(got, two)
        assert np.array_equal(got, expected(o, X, W, idx=idx))
    finally:
        g.close()


def test_output_handle_reused_and_counters():
    """two calls into the same output range (the second overwrites the first), and the OperationsCount counters of one call = those of the two steps"""
    name, K, O = "tiny", 7, 4
    o, g = fresh_context(name)
    try:
        t = PARAMS[name]["t"]
        rng = np.random.default_rng(0xC0)
        W1, W2 = res(small_weights(rng, O, K, t, 3000), t), res(small_weights(rng, O, K, t, 3000), t)
        W1[0, 0] = 0
        X, Y = inputs(o, K, 1), inputs(o, K, 2)
        hx, hy, out, sq, ref = g.ct_alloc(K), g.ct_alloc(K), g.ct_alloc(O), g.ct_alloc(K), g.ct_alloc(O)
        g.ct_upload(hx, 0, X)
        g.ct_upload(hy, 0, Y)
        p1, p2 = g.gemm_plan(W1), g.gemm_plan(W2)
        g.stats(reset=True)
        g.square_gemm(p1, hx, 0, out, 0)
        one = g.stats(reset=True)
        first = g.ct_download(out, 0, O)
        g.square_gemm(p2, hy, 0, out, 0)
        second = g.ct_download(out, 0, O)
        assert g.get_option("square_gemm_fused") == 2
        g.stats(reset=True)
        g.mul_relin(hx, 0, hx, 0, sq, 0, K)
        g.gemm_apply(p1, sq, ref, 0)
        two = g.stats(reset=True)
        assert {c: one[c] for c in COUNTERS} == {c: two[c] for c in COUNTERS}
        assert one["Multiplication"] == K and one["Relinarization"] == K and one["PlainMultiplication"] == O * K - 1
        assert np.array_equal(first, expected(o, X, W1))
        assert np.array_equal(second, expected(o, Y, W2))
        with pytest.raises(Exception):
            g.square_gemm(p1, hx, 0, hx, 0)                          # in place: refused, nothing written
    finally:
        g.close()
