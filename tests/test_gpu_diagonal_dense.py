"""hewrapper.DIAGONAL_DENSE on the device: Mul(..., ForceDenseFormat=True) by generalized diagonals (cn_mul_plain_sum between baby and giant steps) at N = 1024
(m = 512) with two plaintext primes.  Small signed integers, so the integer model is exact: every one of the N decrypted slots equals W v, zero at R and above; the
default path decrypts to the same slots; and the final ciphertext words equal those of the same wrapper path on the CPU backend from the same input ciphertexts
and keys.  A 3 x 1000 matrix is declined by the count rule and gives the default path's words.  The flag is switched on inside the tests only."""
import numpy as np
import pytest

import diag_helpers as dh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def factories():
    g, c = dh.make_factory("gpu"), dh.make_factory("cpu")
    ge, ce = g.AllocateComputationEnv(), c.AllocateComputationEnv()
    for a, b in zip(ge.Environments, ce.Environments):               # the same keys on both sides (the harness seeds its key generator with the prime)
        assert np.array_equal(a.client.relin_key(), b.client.relin_key())
    return g, ge, c, ce


def operands(factories, W, v):
    """the matrix on both backends and ONE encryption of v, carried word for word to the other side"""
    from cryptonets_amd.hewrapper import EMatrixFormat, EVectorFormat
    g, ge, c, ce = factories
    mg, mc = (f.GetPlainMatrix(W.astype(float), EMatrixFormat.RowMajor, 1.0) for f in (g, c))
    vg, vc = (f.GetEncryptedVector(v.astype(float), EVectorFormat.dense, 1.0) for f in (g, c))
    for i, (a, b) in enumerate(zip(ge.Environments, ce.Environments)):
        x, y = vg.eVectors[i].encData, vc.eVectors[i].encData
        b.ctx.ct_upload(y.buf.h, y.first, a.ctx.ct_download(x.buf.h, x.first, 1))
    return mg, vg, mc, vc


@pytest.mark.parametrize("R,dim", dh.SHAPES + [(300, 900)])          # (300 x 900: both column classes complete - the giant steps of both fold together, as at CIFAR shapes)
def test_diagonal_path_equals_the_integer_model_the_default_path_and_the_cpu_words(factories, monkeypatch, R, dim):
    from cryptonets_amd import hewrapper
    g, ge, c, ce = factories
    W, v = dh.weights(R, dim, R + dim), dh.vector(dim, R + dim)
    mg, vg, mc, vc = operands(factories, W, v)
    base = mg.Mul(vg, ge, ForceDenseFormat=True)                     # flag off: the default path
    calls = []
    for e in ge.Environments:
        monkeypatch.setattr(e.ctx, "mul_plain_sum", lambda *a, _f=e.ctx.mul_plain_sum, **kw: (calls.append(1), _f(*a, **kw))[1], raising=False)
    monkeypatch.setattr(hewrapper, "DIAGONAL_DENSE", True)
    assert mg.DiagonalDenseWins(vg, ge)
    out = mg.Mul(vg, ge, ForceDenseFormat=True)
    assert len(calls) == len(ge.Environments), "one cn_mul_plain_sum per plaintext prime"
    want = dh.expected_slots(W, v)
    got = dh.decrypted_slots(out, ge)
    assert np.array_equal(got, want) and not got[R:].any()
    assert np.array_equal(dh.decrypted_slots(base, ge), want)
    assert (out.Scale, out.Dim, out.Format) == (base.Scale, base.Dim, base.Format) and out.Dim == R
    ref = mc.Mul(vc, ce, ForceDenseFormat=True)                      # the same wrapper path on the oracle: mul_plain + add_many per group
    for a, b in zip(dh.words(out, ge), dh.words(ref, ce)):
        assert np.array_equal(a, b)
    for m in (mg, mc):
        m.Dispose()


def test_a_wide_three_row_matrix_is_declined_and_keeps_the_default_words(factories, monkeypatch):
    from cryptonets_amd import hewrapper
    g, ge, c, ce = factories
    W, v = dh.weights(3, 1000, 5), dh.vector(1000, 5)
    mg, vg, mc, vc = operands(factories, W, v)
    base = mg.Mul(vg, ge, ForceDenseFormat=True)
    monkeypatch.setattr(hewrapper, "DIAGONAL_DENSE", True)
    assert not mg.DiagonalDenseWins(vg, ge) and mg.DiagonalDenseCounts(vg, ge)["choice"] == "default"
    out = mg.Mul(vg, ge, ForceDenseFormat=True)
    for a, b in zip(dh.words(out, ge), dh.words(base, ge)):
        assert np.array_equal(a, b)
    assert np.array_equal(dh.decrypted_slots(out, ge), dh.expected_slots(W, v))
    assert "_diagplan" not in mg.__dict__
    for m in (mg, mc):
        m.Dispose()


def test_rotation_steps_of_the_diagonal_path_are_recorded(factories, monkeypatch):
    """cn_set_option("record_steps") - what networks.rotation_steps reads - sees the baby steps 1, 2, .., B / 2, the giant steps and the column swap by itself"""
    from cryptonets_amd import hewrapper
    g, ge, c, ce = factories
    R, dim = 512, 512
    W, v = dh.weights(R, dim, 8), dh.vector(dim, 8)
    mg, vg, mc, vc = operands(factories, W, v)
    monkeypatch.setattr(hewrapper, "DIAGONAL_DENSE", True)
    ctx = ge.Environments[0].ctx
    ctx.set_option("record_steps", 1)
    try:
        mg.Mul(vg, ge, ForceDenseFormat=True)
        steps, columns = ctx.rotation_steps()
    finally:
        ctx.set_option("record_steps", 0)
    plan = mg._diagonal_plan(0, ge.Environments[0])[0]
    assert plan.babies_by_doubling and plan.giants_by_folding and plan.classes == [0]
    want = {1 << s for s in range(plan.B.bit_length() - 1)} | {(1 << s) * plan.B for s in range(plan.Gs.bit_length() - 1)}
    assert {int(s) % 512 for s in steps} == {s % 512 for s in want} and not columns      # 512 x 512: no c = 1 diagonal, so no column swap
    for m in (mg, mc):
        m.Dispose()
