"""The clipped + residual weight form of the matrix-core GEMMs (gemm_residual_form, cn_gemm_plan.h; k_scalar_gemm_mfma / k_digit_gemm_mfma <1, .., GemmResidual>)
on the device, word for word against the same plan with the form switched off (CN_GEMM_RESIDUAL=0 while the plan is built: base-256 planes, P = 2) and against the
CPU oracle.  The "on" plan is built under CN_GEMM_RESIDUAL=2, the form up to half the K steps: by default the planner stops at one residual step in eight, which
layers of two to four K steps never reach.

Every case builds both plans over the same weights and runs, for each: cn_gemm_plan_apply (the ciphertext form), cn_square_gemm in the fused form ("sg_prefloor" = 0:
the ciphertext form and the digit GEMM) and in the pre-floor form ("sg_prefloor" = 2: the Bsk form, the y form and the digit GEMM).  All six results must be the words
of the oracle's mul_relin_batch + scalar_gemm + add_plain_batch.

Shapes: N = 1024, three limbs ("tiny"); M = 16, 33, 40 (one and two output tiles, the last one partial); K = 33, 70, 100 (two, three and four K steps - one and two
steps behind a whole turn of the kernels' three-set ring, and a turn plus the residual steps).  Weights: test_gemm_residual_plan.device_weights - mostly |w| <= 20, a
handful in 128..254 of both signs, one in the last K slot, one row with a residual wherever any row has one; kres = 1, 1 and 2 (half the steps at K = 100).  That
module plans the same weights with this ring's parameters on the CPU and asserts that they take the form with these kres (the library has no counter for it, and
the counter names are pinned by tests/test_options.py).  "device-two-lists": two gather lists of 20 outputs each over the same 100 inputs, one with a padded tap and
every residual (kres = 1), the other without any (kres = 0 inside a plan of the form).  One more case keeps |w| <= 127: one plane, no residual, whatever the switch
says.  Not run on the device: the address-table instantiation <1, true, GemmResidual>, which only a flush of the deferred queue launches."""
import numpy as np
import pytest

from conftest import PARAMS
from test_gemm_residual_plan import DEVICE_LISTS, DEVICE_LISTS_W, DEVICE_SHAPES, device_weights, rows
from test_square_gemm import inputs, res

pytestmark = pytest.mark.gpu

_ring = {}


def ring():
    """(oracle, its 100 inputs, their relinearized squares): once"""
    from oracle.cno import Oracle
    if not _ring:
        p = PARAMS["tiny"]
        o = Oracle(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"])
        o.keygen(11, galois=False)
        X = inputs(o, 100, 0x2E5)
        X.setflags(write=False)
        sq = o.mul_relin_batch(X, X)
        sq.setflags(write=False)
        _ring["r"] = (o, X, sq)
    return _ring["r"]


def run_forms(g, monkeypatch, X, sq, W, O, bias, idx=None):
    """{(switch, call): words} of cn_gemm_plan_apply on the squares and of cn_square_gemm in both forms, for the plan with the form on and switched off"""
    h, hs, dst, bh = g.ct_alloc(len(X)), g.ct_alloc(len(X)), g.ct_alloc(O + 1), g.pt_alloc(O)
    g.ct_upload(h, 0, X)
    g.ct_upload(hs, 0, sq)
    g.pt_upload(bh, 0, bias)
    out = {}
    for switch in ("on", "off"):
        monkeypatch.setenv("CN_GEMM_RESIDUAL", "0" if switch == "off" else "2")
        plan = g.gemm_plan(W, idx=idx, bias_pt=bh, bias_idx=np.arange(O, dtype=np.int32))
        monkeypatch.delenv("CN_GEMM_RESIDUAL", raising=False)
        g.gemm_apply(plan, hs, dst, 1)
        out[switch, "apply"] = g.ct_download(dst, 1, O)
        for mode, call in ((0, "fused"), (2, "prefloor")):
            g.set_option("sg_prefloor", mode)
            p0, f0, d0 = g.get_option("square_gemm_prefloor"), g.get_option("square_gemm_fused"), g.get_option("digit_gemm_mfma")
            g.square_gemm(plan, h, 0, dst, 1)
            out[switch, call] = g.ct_download(dst, 1, O)
            steps = (g.get_option("square_gemm_prefloor") - p0, g.get_option("square_gemm_fused") - f0, g.get_option("digit_gemm_mfma") - d0)
            assert steps == (mode // 2, 1, 1), (switch, call, steps)                # the form asked for, one key switch per output, the digit GEMM on the matrix cores
        g.set_option("sg_prefloor", 1)
        g.free(plan)
    for x in (h, hs, dst, bh):
        g.free(x)
    return out


def check(monkeypatch, W, O, K, idx=None):
    from cryptonets_amd._native import Context
    o, X, sq = ring()
    p = PARAMS["tiny"]
    t = p["t"]
    g = Context(p["n"], t, q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)
    try:
        g.set_relin_key(o.relin_key())
        bias = np.stack([o.encode(np.full(o.n, (v * 977 + 1) % t, dtype=np.uint64)) for v in range(O)])
        want = o.add_plain_batch(o.scalar_gemm(sq[:K], res(W, t), idx), bias)
        got = run_forms(g, monkeypatch, X[:K], sq[:K], res(W, t), O, bias, idx)
        for key in sorted(got):
            assert np.array_equal(got[key], got["off", "apply"]), key
            assert np.array_equal(got[key], want), key
    finally:
        g.close()


@pytest.mark.parametrize("M,K", DEVICE_SHAPES)
def test_words_of_the_switched_off_plan_and_of_the_oracle(monkeypatch, M, K):
    check(monkeypatch, np.array(device_weights(M, K)), M, K)


def test_two_gather_lists_one_of_them_without_a_residual(monkeypatch):
    check(monkeypatch, np.array(DEVICE_LISTS_W), 40, 100, idx=np.array(DEVICE_LISTS, dtype=np.int32))


def test_one_plane_without_residual_is_unchanged(monkeypatch):
    """max |w| = 127: the plan is not in the form (P = 1, kres nowhere) with the switch on or off"""
    M, K = 33, 70
    check(monkeypatch, np.array(rows(M, K, 3, [(3, 7, 127), (9, 69, -127)])), M, K)
