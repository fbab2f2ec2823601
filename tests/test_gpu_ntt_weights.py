"""hewrapper.NTT_WEIGHTS on the device: the weight plaintexts of a row-major matrix - rows, one-hot masks, pre-rotated diagonals - resident in NTT form
(cn_pt_transform).  The 37 x 700 matrix of tests/test_gpu_diagonal_dense.py at N = 1024, three limbs, two plaintext primes: Mul(..., ForceDenseFormat=True) under
DIAGONAL_DENSE and RowsDotProduct (with ForceOutputInColumns, and with a bias) give the SAME ciphertext words with the flag off and on; with it on, a call on the
resident arrays runs no transform of a plaintext (the device's transform counter), a second call allocates nothing, and Dispose returns every handle.  The flags
are switched on inside the tests only."""
import numpy as np
import pytest

import diag_helpers as dh
from test_gpu_diagonal_dense import factories, operands          # noqa: F401 (the module-scoped fixture and its operand builder)

pytestmark = pytest.mark.gpu

R, DIM = 37, 700


def fwd(env):
    return [e.ctx.stats()["ntt_forward_limbs"] for e in env.Environments]


def live(env):
    return [e.ctx.live_handles() for e in env.Environments]


def both_forms(monkeypatch, env, call):
    """call() with NTT_WEIGHTS off, then on (twice: the second run finds the arrays resident): the three results' words, the forward limb transforms of the
    resident runs (off, on) per prime, and the handles the second resident run left behind"""
    from cryptonets_amd import hewrapper
    monkeypatch.setattr(hewrapper, "NTT_WEIGHTS", False)
    call()                                                           # builds the coefficient-form caches
    f0 = fwd(env)
    off = dh.words(call(), env)
    f1 = fwd(env)
    monkeypatch.setattr(hewrapper, "NTT_WEIGHTS", True)
    first = dh.words(call(), env)                                    # builds the NTT-form caches
    h0, f2 = live(env), fwd(env)
    keep = call()
    on = dh.words(keep, env)
    h1, f3 = live(env), fwd(env)
    for a, b, c in zip(off, first, on):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    return [b - a for a, b in zip(f0, f1)], [b - a for a, b in zip(f2, f3)], [b - a for a, b in zip(h0, h1)]


def test_diagonal_dense_words_and_no_plaintext_transform(factories, monkeypatch):
    from cryptonets_amd import hewrapper
    g, ge, c, ce = factories
    W, v = dh.weights(R, DIM, R + DIM), dh.vector(DIM, R + DIM)
    start = live(ge)
    mg, vg, mc, vc = operands(factories, W, v)
    monkeypatch.setattr(hewrapper, "DIAGONAL_DENSE", True)
    assert mg.DiagonalDenseWins(vg, ge)
    sums = {}                                                        # per prime: forward limb transforms of each cn_mul_plain_sum call
    for i, e in enumerate(ge.Environments):
        def counted(*a, _f=e.ctx.mul_plain_sum, _c=e.ctx, _i=i, **kw):
            before = _c.stats()["ntt_forward_limbs"]
            _f(*a, **kw)
            sums.setdefault(_i, []).append(_c.stats()["ntt_forward_limbs"] - before)
        monkeypatch.setattr(e.ctx, "mul_plain_sum", counted, raising=False)
    held = []
    off, on, grown = both_forms(monkeypatch, ge, lambda: held.append(mg.Mul(vg, ge, ForceDenseFormat=True)) or held[-1])
    assert np.array_equal(dh.decrypted_slots(held[-1], ge), dh.expected_slots(W, v))
    k = len(dh.TINY_Q)
    for i, e in enumerate(ge.Environments):
        plan = mg._diagonal_plan(i, e)[0]
        assert len(sums[i]) == 4 and sums[i][2] == sums[i][3] == len(plan.babies) * 2 * k      # NTT form: the rotated inputs' transforms and nothing else
        assert sums[i][1] - sums[i][3] >= plan.terms * 2 * k         # the coefficient form transforms every diagonal in both polynomials' blocks on top
        assert off[i] - on[i] >= plan.terms * 2 * k
        assert e.ctx.get_option("ptn_sum") >= 2
        assert grown[i] == 1                                         # the second resident call: its result and nothing else
    for x in held:
        x.Dispose()
    for m in (mg, mc):
        m.Dispose()
    vg.Dispose()
    assert live(ge) == start


@pytest.mark.parametrize("columns", [True, False], ids=["output-in-columns", "bias"])
def test_rows_dot_product_words_and_no_plaintext_transform(factories, monkeypatch, columns):
    from cryptonets_amd.hewrapper import EMatrixFormat
    g, ge, c, ce = factories
    W, v = dh.weights(R, DIM, 11), dh.vector(DIM, 11)
    start = live(ge)
    mg, vg, mc, vc = operands(factories, W, v)
    bias = None if columns else g.GetPlainMatrix(dh.weights(R, DIM, 12).astype(float), EMatrixFormat.RowMajor, 1.0)
    held = []

    def call():
        out = mg.RowsDotProduct(vg, ge, ForceOutputInColumns=columns, bias=bias)
        held.append(out)
        return out if columns else out[0]                            # (row 0 stands for the rows: they share one array per prime)

    def all_rows(out):
        return [e.ctx.ct_download(out[0].eVectors[i].encData.buf.h, 0, R) for i, e in enumerate(ge.Environments)]

    off, on, grown = both_forms(monkeypatch, ge, call)
    if not columns:
        for a, b in zip(all_rows(held[1]), all_rows(held[-1])):      # every row, flag off against flag on
            assert np.array_equal(a, b)
    k = len(dh.TINY_Q)
    for i, e in enumerate(ge.Environments):
        # off: every row plaintext in both polynomials' blocks (and k limbs per mask); on: the ciphertext's transforms and the key switches' alone
        assert off[i] - on[i] >= R * 2 * k + (R * k if columns else 0)
        assert e.ctx.get_option("ptn_bcast") >= 2
        assert grown[i] == 1
    for out in held:
        for x in ([out] if columns else out):
            x.Dispose()
    for m in (mg, mc) + (() if bias is None else (bias,)):
        m.Dispose()
    vg.Dispose()
    assert live(ge) == start
