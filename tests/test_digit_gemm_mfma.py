"""The digit GEMM of cn_square_gemm on the int8 matrix cores (k_digit_gemm_mfma) against the FP64 form, the library's two separate steps and the CPU oracle.

The digit GEMM has TWO forms.  Where the plan's own GEMM takes the matrix cores (small weights, >= 16 outputs per gather list, 3 K < 2^17, limbs of at most 46 bits)
and a digit splits into two int8 pieces (dbc <= 14), the weight-combined digit polynomials S are contracted on v_mfma_i32_32x32x32_i8 from the plan's weight
fragments; everywhere else - fewer than 16 outputs, K at the bound, "digit_mfma" = 0 when the plan was made - the FP64 kernel k_digit_gemm runs as before.  Both
give the same exact doubles S, so the ciphertext words do not depend on the form.

Every case asserts: "square_gemm_fused" rose by 1; "digit_gemm_mfma" rose by 1 where the matrix form is expected and by 0 where it is not; the words equal
cn_mul_relin + cn_gemm_plan_apply and the same call planned with "digit_mfma" = 0; where the oracle is named, also mul_relin_batch + scalar_gemm.

Shapes: ring "tiny" (N = 1024, three limbs of 36-37 bits = 4 digits at dbc 10: two digit groups of the kernel, the second with one digit) for the K tails of the
three-set register ring (1 partial step, 2 steps, 3 steps, 4 steps), the output tiles (half a tile; two tiles, one row in the second, two waves idle; five tiles = two tile
groups), one to three weight digit planes with the recode edges 127 / 128 / 32639 / 32640, digit widths 12 and 7 (4 and 6 digits per limb), gather lists with padded
taps and padding members; ring "c3" (CryptoNets: N = 8192, five limbs of five digits) for two digit groups of 3 + 2, the fused key switch and the i32 head-room at the
largest K the form accepts.  The squared inputs of the oracle are computed once per ring and shared.
"""
import numpy as np
import pytest

from conftest import PARAMS
from test_square_gemm import expected, fresh_context, inputs, res, small_weights

pytestmark = pytest.mark.gpu

_squares = {}


def squares(o, name, count):
    """(uniform inputs, their relinearized squares by the oracle), computed once per ring for the largest count any case asks for"""
    need = {"tiny": 100, "c3": 40}[name]
    assert count <= need
    if name not in _squares:
        X = inputs(o, need, 0xD16 + need)
        X.setflags(write=False)
        sq = o.mul_relin_batch(X, X)
        sq.setflags(write=False)
        _squares[name] = (X, sq)
    X, sq = _squares[name]
    return X[:count], sq[:count]


def context_at(name, dbc):
    """ring `name` with another decomposition bit count: its own oracle (keys depend on the digit width) and context"""
    from cryptonets_amd._native import Context
    from oracle.cno import Oracle
    p = PARAMS[name]
    o = Oracle(p["n"], p["t"], q=p["q"], dbc=dbc, gdbc=p["gdbc"])
    o.keygen(11, galois=False)
    g = Context(p["n"], p["t"], q=p["q"], dbc=dbc, gdbc=p["gdbc"], device=0)
    g.set_relin_key(o.relin_key())
    return o, g


def run_forms(g, X, W, O, idx=None, bias=None, out_extra=0):
    """words of cn_square_gemm as planned by default, planned with digit_mfma = 0, and of the two library steps; the counters' steps of the two fused calls"""
    h, sq = g.ct_alloc(len(X)), g.ct_alloc(len(X))
    a, z, b = g.ct_alloc(O + out_extra), g.ct_alloc(O + out_extra), g.ct_alloc(O)
    g.ct_upload(h, 0, X)
    bh = 0
    if bias is not None:
        bh = g.pt_alloc(len(bias))
        g.pt_upload(bh, 0, bias)
    bidx = np.arange(O, dtype=np.int32) if bias is not None else None
    plan = g.gemm_plan(W, idx=idx, bias_pt=bh, bias_idx=bidx)
    g.set_option("digit_mfma", 0)
    plan0 = g.gemm_plan(W, idx=idx, bias_pt=bh, bias_idx=bidx)
    g.set_option("digit_mfma", 1)
    steps = []
    for p, out in ((plan, a), (plan0, z)):
        f0, m0 = g.get_option("square_gemm_fused"), g.get_option("digit_gemm_mfma")
        g.square_gemm(p, h, 0, out, out_extra)
        steps.append((g.get_option("square_gemm_fused") - f0, g.get_option("digit_gemm_mfma") - m0))
    g.mul_relin(h, 0, h, 0, sq, 0, len(X))
    g.gemm_apply(plan, sq, b, 0)
    words = g.ct_download(a, out_extra, O), g.ct_download(z, out_extra, O), g.ct_download(b, 0, O)
    for x in (h, sq, a, z, b, plan, plan0):
        g.free(x)
    return words, steps


def check(g, X, W, O, matrix, oracle=None, **kw):
    """the three assertions of every case; oracle: the expected words, or None"""
    (got, fp64, two), steps = run_forms(g, X, W, O, **kw)
    assert steps[0][0] == 1 and steps[1][0] == 1, "both calls are meant to run one key switch per output"
    assert steps[0][1] == (1 if matrix else 0), "form of the digit GEMM as planned by default"
    assert steps[1][1] == 0, "a plan made with digit_mfma = 0 runs the FP64 form"
    assert np.array_equal(got, two)
    assert np.array_equal(got, fp64)
    if oracle is not None:
        assert np.array_equal(got, oracle)


@pytest.mark.parametrize("K,wmax", [(3, 127), (33, 127), (70, 6144), (100, 6144)])
def test_k_tails_and_the_register_ring(K, wmax):
    """one partial K step, two steps, a full turn of the three-set ring, a turn plus one step; one weight plane (|w| <= 127) and two (up to t / 2 = 6144)"""
    name, O = "tiny", 16
    o, g = fresh_context(name)
    try:
        t = PARAMS[name]["t"]
        W = small_weights(np.random.default_rng(0xA0 + K), O, K, t, wmax)
        W[0, :] = wmax
        X, sq = squares(o, name, K)
        check(g, X, res(W, t), O, True, oracle=o.scalar_gemm(sq, res(W, t)))
    finally:
        g.close()


@pytest.mark.parametrize("O", [16, 33, 130])
def test_output_tiles(O):
    """half a tile; two tiles, the second with one row and two waves without a tile; five tiles in two tile groups.  Row o = (o + 1) (-1)^o times the all-ones
    row: every output differs, a swapped row / column store cannot pass"""
    name, K = "tiny", 40
    o, g = fresh_context(name)
    try:
        t = PARAMS[name]["t"]
        W = np.outer((np.arange(O) + 1) * np.where(np.arange(O) % 2, -1, 1), np.ones(K, dtype=np.int64))
        X, sq = squares(o, name, K)
        check(g, X, res(W, t), O, True, oracle=o.scalar_gemm(sq, res(W, t)) if O <= 33 else None)
    finally:
        g.close()


@pytest.mark.parametrize("case", ["recode_edges", "three_planes"])
def test_weight_planes_and_recode_edges(case):
    """rows of 127, -127, 128, -128, 32639, -32639, 32640, -32640 (the last values of one / two signed byte digits and the first of the next plane), the rest random
    within +-32639; and |w| up to 2^19 - 1.  Row sums stay below tiny's bound sum |w| < 2^25.  (tiny's ring and moduli with the plain modulus 2101249, the first
    prime = 1 mod 2048 above 2^21: tiny's own 12289 has no weights beyond 6144.)"""
    name, K, O = "tiny", 40, 16
    p = PARAMS[name]
    from cryptonets_amd._native import Context
    from oracle.cno import Oracle
    t = 2101249
    o = Oracle(p["n"], t, q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"])
    o.keygen(11, galois=False)
    g = Context(p["n"], t, q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)
    try:
        g.set_relin_key(o.relin_key())
        rng = np.random.default_rng(0xED6E)
        if case == "recode_edges":
            W = small_weights(rng, O, K, t, 32639)
            for r, v in enumerate((127, -127, 128, -128, 32639, -32639, 32640, -32640)):
                W[r, :] = v
        else:
            W = small_weights(rng, O, K, t, (1 << 19) - 1)
            W[0, :] = (1 << 19) - 1
            W[1, ::2] = -((1 << 19) - 1)
        assert np.abs(W).sum(axis=1).max() < 1 << 25
        X = inputs(o, K, 0xED)
        check(g, X, res(W, t), O, True, oracle=expected(o, X, res(W, t)))
    finally:
        g.close()


@pytest.mark.parametrize("K,O", [(8, 40), (40, 100)])
def test_cryptonets_ring(K, O):
    """five limbs of five digits: digit groups of 3 and 2; 40 outputs = two tiles, 100 = four, the last with 4 rows"""
    name = "c3"
    o, g = fresh_context(name)
    try:
        t = PARAMS[name]["t"]
        W = small_weights(np.random.default_rng(0xC3 + K), O, K, t, 32639)
        W[0, :] = 32639
        W[1, ::2] = -32639
        X, sq = squares(o, name, K)
        check(g, X, res(W, t), O, True, oracle=o.scalar_gemm(sq, res(W, t)))
    finally:
        g.close()


@pytest.mark.parametrize("dbc", [12, 7])
def test_another_digit_width(dbc):
    """dbc 12: pieces lo in -128..127, hi in 0..16; dbc 7: hi in 0..1 and six digits per limb.  Both are within the split's dbc <= 14: the matrix form runs"""
    name, K, O = "tiny", 40, 16
    o, g = context_at(name, dbc)
    try:
        t = PARAMS[name]["t"]
        W = small_weights(np.random.default_rng(0xDB + dbc), O, K, t, 1000)
        assert np.abs(W).sum(axis=1).max() * ((1 << dbc) - 1) < min(o.q) // 2
        X = inputs(o, K, 0xDB)
        check(g, X, res(W, t), O, True, oracle=expected(o, X, res(W, t)))
    finally:
        g.close()


def test_gather_lists_zero_weights_bias_and_output_offset():
    """three gather lists with padded taps (-1): 16 outputs on the first, one on each of the others (their 15 padding members store nothing); zero weights, a weight
    on a padded tap, a bias per output, the outputs at an offset of their handle"""
    name, K, O = "tiny", 6, 18
    o, g = fresh_context(name)
    try:
        t = PARAMS[name]["t"]
        rng = np.random.default_rng(0x6A8)
        idx = np.array([[0, 1, 2, -1, 4, 5]] * 16 + [[6, 5, -1, 3, 2, -1]] + [[3, -1, 6, 0, 1, 4]], dtype=np.int32)
        W = small_weights(rng, O, K, t, 1000)
        W[0, 1] = 0
        W[3, 0] = 0
        W[16, 5] = 77                                                # a weight on a padded tap counts for nothing
        W[17, 0] = 0
        X = inputs(o, 7, 0x77)
        bias = np.stack([o.encode(np.full(o.n, v % t, dtype=np.uint64)) for v in range(1, O + 1)])
        check(g, X, res(W, t), O, True, oracle=expected(o, X, res(W, t), idx=idx, bias=bias), idx=idx, bias=bias, out_extra=2)
    finally:
        g.close()


def test_accumulator_head_room():
    """the largest K the matrix form accepts (a multiple of 32 under 3 K < 2^17), every weight +-32639 = byte digits (127, 127) / (-127, -127), the first input with every
    residue q - 1: rows of one sign drive the i32 diagonals as far as these inputs can.  Against the FP64 form and the two steps only (the oracle would take minutes)"""
    name, K, O = "c3", 43680, 16
    o, g = fresh_context(name)
    try:
        t = PARAMS[name]["t"]
        assert 3 * K < 1 << 17 <= 3 * (K + 32) and K * 32639 * 1023 < min(o.q) // 2
        idx = np.tile(np.arange(4, dtype=np.int32), (O, K // 4))
        W = np.where(np.random.default_rng(0x43680).integers(0, 2, size=(O, K)) == 1, 32639, -32639)
        W[0, :] = 32639
        W[1, :] = -32639
        X = inputs(o, 4, 0xACC)
        check(g, X, res(W, t), O, True, idx=idx)
    finally:
        g.close()


def test_fall_back_at_the_k_bound():
    """32 terms more: 3 K >= 2^17, the plan's GEMM and its digit GEMM take their FP64 forms; still one key switch per output"""
    name, K, O = "tiny", 43712, 16
    o, g = fresh_context(name)
    try:
        t = PARAMS[name]["t"]
        assert 3 * K >= 1 << 17 and K * 1023 < min(o.q) // 2
        idx = np.tile(np.arange(4, dtype=np.int32), (O, K // 4))
        W = np.where(np.random.default_rng(0x43712).integers(0, 2, size=(O, K)) == 1, 1, -1)
        X = inputs(o, 4, 0xFB)
        (got, fp64, two), steps = run_forms(g, X, res(W, t), O, idx=idx)
        assert steps == [(1, 0), (1, 0)]
        assert np.array_equal(got, two)
        assert np.array_equal(got, fp64)
        assert np.array_equal(got[:2], expected(o, X, res(W[:2], t), idx=idx[:2]))
    finally:
        g.close()


def test_switch_affects_plans_made_after_it():
    name, K, O = "tiny", 40, 16
    o, g = fresh_context(name)
    try:
        t = PARAMS[name]["t"]
        assert g.get_option("digit_mfma") == 1 and g.get_option("digit_gemm_mfma") == 0
        W = res(small_weights(np.random.default_rng(0x5A), O, K, t, 1000), t)
        X, sq = squares(o, name, K)
        want = o.scalar_gemm(sq, W)
        h, out = g.ct_alloc(K), g.ct_alloc(O)
        g.ct_upload(h, 0, X)
        before = g.gemm_plan(W)
        g.set_option("digit_mfma", 0)
        assert g.get_option("digit_mfma") == 0
        after = g.gemm_plan(W)
        for plan, step in ((after, 0), (before, 1)):                 # the switch is still off: a plan made before keeps its form
            m0, f0 = g.get_option("digit_gemm_mfma"), g.get_option("square_gemm_fused")
            g.square_gemm(plan, h, 0, out, 0)
            assert g.get_option("square_gemm_fused") - f0 == 1
            assert g.get_option("digit_gemm_mfma") - m0 == step
            assert np.array_equal(g.ct_download(out, 0, O), want)
        with pytest.raises(Exception):
            g.set_option("digit_gemm_mfma", 1)                       # the counter is read-only
    finally:
        g.close()
