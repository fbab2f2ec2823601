"""hewrapper.DEVICE_DIAGONAL_PLAN on the device: the diagonal plan of a dense layer built by cn_diag_scan + diagonal.plan_from_flags + ONE cn_diag_encode gives the
ciphertext words of the host-built plan (decode_batch, numpy, encode_batch per chunk) from the same input ciphertext - with NTT_WEIGHTS off and on -, the same plan,
an array of exactly plan.terms plaintexts, no decode_batch / encode_batch on its way, and nothing left behind after Dispose.  N = 1024, two plaintext primes
(diag_helpers); the switches are set inside the tests only."""
import numpy as np
import pytest

import diag_helpers as dh

pytestmark = pytest.mark.gpu
ATTRS = ("n", "m", "R", "Dim", "B", "Gs", "babies", "groups", "grp_off", "ct_idx")


def banded(R, dim, seed):
    W = dh.weights(R, dim, seed)
    r, x = np.indices(W.shape)
    W[(r - x) % 7 != 0] = 0
    return W


@pytest.fixture(scope="module")
def gpu():
    f = dh.make_factory("gpu")
    return f, f.AllocateComputationEnv()


@pytest.mark.parametrize("ntt", [False, True])
@pytest.mark.parametrize("R,dim,band", [(R, dim, False) for (R, dim) in dh.SHAPES + [(300, 900)]] + [(300, 900, True)])
def test_device_built_plan_gives_the_words_of_the_host_built_plan(gpu, monkeypatch, R, dim, band, ntt):
    from cryptonets_amd import hewrapper
    from cryptonets_amd.hewrapper import EMatrixFormat, EVectorFormat
    f, env = gpu
    W = banded(R, dim, R + dim) if band else dh.weights(R, dim, R + dim)
    v = dh.vector(dim, R + dim)
    ctxs = [e.ctx for e in env.Environments]
    live0 = [c.live_handles() for c in ctxs]
    mat = f.GetPlainMatrix(W.astype(float), EMatrixFormat.RowMajor, 1.0)
    vec = f.GetEncryptedVector(v.astype(float), EVectorFormat.dense, 1.0)
    monkeypatch.setattr(hewrapper, "DIAGONAL_DENSE", True)
    monkeypatch.setattr(hewrapper, "NTT_WEIGHTS", ntt)
    calls = {"decode_batch": 0, "encode_batch": 0, "diag_scan": 0, "diag_encode": 0}
    for c in ctxs:
        for name in calls:
            def counted(*a, _f=getattr(c, name), _n=name, **kw):
                calls[_n] += 1
                return _f(*a, **kw)
            monkeypatch.setattr(c, name, counted, raising=False)
    monkeypatch.setattr(hewrapper, "DEVICE_DIAGONAL_PLAN", False)
    host = mat.DiagonalDense(vec, env) if band else mat.Mul(vec, env, ForceDenseFormat=True)
    assert calls["decode_batch"] == len(ctxs) and calls["encode_batch"] >= len(ctxs) and calls["diag_scan"] == 0, calls
    for name in calls:
        calls[name] = 0
    monkeypatch.setattr(hewrapper, "DEVICE_DIAGONAL_PLAN", True)
    dev = mat.DiagonalDense(vec, env) if band else mat.Mul(vec, env, ForceDenseFormat=True)
    assert calls == {"decode_batch": 0, "encode_batch": 0, "diag_scan": len(ctxs), "diag_encode": len(ctxs)}, calls
    for a, b in zip(dh.words(dev, env), dh.words(host, env)):
        assert np.array_equal(a, b)
    assert np.array_equal(dh.decrypted_slots(dev, env), dh.expected_slots(W, v))
    for i, e in enumerate(env.Environments):
        monkeypatch.setattr(hewrapper, "DEVICE_DIAGONAL_PLAN", False)
        hp, hpts = mat._diagonal_plan(i, e)
        monkeypatch.setattr(hewrapper, "DEVICE_DIAGONAL_PLAN", True)
        dp, dpts = mat._diagonal_plan(i, e)
        assert dpts is not hpts, "the cache key carries the switch"
        for attr in ATTRS:
            assert getattr(dp, attr) == getattr(hp, attr), attr
        assert dpts.count == dp.terms and dpts.buf.count == dp.terms, "exactly plan.terms plaintexts"
        assert hpts.buf.count >= hp.terms
        if band:
            assert dp.terms < hpts.buf.count, "the host route allocates the structural bound"
        down = e.ctx.ptn_download if ntt else e.ctx.pt_download
        assert np.array_equal(down(dpts.h, dpts.first, dp.terms), down(hpts.h, hpts.first, hp.terms))
    assert calls == {"decode_batch": 0, "encode_batch": 0, "diag_scan": len(ctxs), "diag_encode": len(ctxs)}, "both plans came out of the cache"
    for x in (host, dev, vec):
        x.Dispose()
    mat.Dispose()
    assert [c.live_handles() for c in ctxs] == live0


def test_a_single_column_matrix_keeps_its_37_diagonals_and_leaks_nothing(gpu, monkeypatch):
    from cryptonets_amd import hewrapper
    from cryptonets_amd.hewrapper import EMatrixFormat, EVectorFormat
    f, env = gpu
    ctxs = [e.ctx for e in env.Environments]
    live0 = [c.live_handles() for c in ctxs]
    W = np.zeros((37, 700))
    W[:, 0] = 1
    mat = f.GetPlainMatrix(W, EMatrixFormat.RowMajor, 1.0)
    monkeypatch.setattr(hewrapper, "DEVICE_DIAGONAL_PLAN", True)
    e = env.Environments[0]
    rows = mat._row_plaintexts(0, e)
    nz = e.ctx.diag_scan(rows.h, rows.first, 37, 700)
    assert int(nz.sum()) == 37 and nz[0, -36:].all() and nz[0, 0]      # column 0 alone: the diagonals (0, -p), p < 37
    plan, pts = mat._diagonal_plan(0, e)
    assert plan.terms == 37 and pts.buf.count == 37
    mat.Dispose()
    assert [c.live_handles() for c in ctxs] == live0
