"""hewrapper.SUMMED_ROTATIONS on the device: the output blocks of Interleave, the selections of Permute and the giant steps of DiagonalDense through
cn_rotate_rows_sum.  N = 1024, the two plaintext primes and the coefficient moduli of tests/diag_helpers.py, keygen / encrypt / decrypt on the device with the
DEFAULT Galois keys (the factory of tests/test_gpu_hoisted_consumers.py): steps without a key of their own run their hops inside the call.

With the switch off nothing moves "ks_summed".  With it on, Interleave (the LoLa shape: 13 columns, shift -1; and 6 columns of 200 values at shift 200 - two output
blocks, one vector split at the half and one at the block boundary, `upper` lists) and Permute (three selections, one of them absent, a step with hops and a step
of 0) return the ciphertext WORDS of the switch-off run.  DiagonalDense on the 37 x 700 layer decrypts to W v mod t with zeros above row 37 in both plan shapes
(B = 256: the giant steps fold; B = 64: zero diagonals leave gaps), and "ks_summed" has moved by one per plaintext prime.  The switch is set inside the tests only
and restored."""
import numpy as np
import pytest

import diag_helpers as dh
from test_gpu_hoisted_consumers import factory

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    F = factory()
    env = F.AllocateComputationEnv()
    yield F, env
    F.FreeComputationEnv(env)


def summed(env):
    return [e.ctx.get_option("ks_summed") for e in env.Environments]


def matrix(F, cols, dim, seed):
    from cryptonets_amd.hewrapper import EMatrixFormat
    data = np.random.default_rng(seed).integers(-3, 4, size=(dim, cols)).astype(float)
    return data, F.GetEncryptedMatrix(data, EMatrixFormat.ColumnMajor, 1)


def blocks_of(vec, env):
    """the words of every block of a result, per plaintext prime"""
    return [e.ctx.ct_download(vec.eVectors[i].encData.buf.h, vec.eVectors[i].encData.first, vec.eVectors[i].encData.count) for i, e in enumerate(env.Environments)]


def all_slots(vec, env):
    """all N slots of a single-block result as residues, per plaintext prime (whatever its registered Dim)"""
    out = []
    for i, e in enumerate(env.Environments):
        a = vec.eVectors[i].encData
        plains = e.client.decrypt_device(a.h, a.first, 1)
        pt = e.ctx.pt_alloc(1)
        try:
            e.ctx.pt_upload(pt, 0, np.asarray(plains)[:1])
            out.append(np.asarray(e.ctx.decode_batch(pt, 0, 1)[0], dtype=np.int64))
        finally:
            e.ctx.free(pt)
    return out


@pytest.mark.parametrize("cols, dim, shift, blocks", [(13, 40, -1, 1), (6, 200, 200, 2)], ids=["lola-13-rows", "two-blocks-with-splits"])
def test_interleave_returns_the_words_of_the_switch_off_run(fx, monkeypatch, cols, dim, shift, blocks):
    from cryptonets_amd import hewrapper
    F, env = fx
    data, m = matrix(F, cols, dim, 3 + dim)
    before = summed(env)
    base = m.Interleave(shift, env)
    assert summed(env) == before, "the switch is off: no summed call"
    monkeypatch.setattr(hewrapper, "SUMMED_ROTATIONS", True)
    out = m.Interleave(shift, env)
    assert summed(env) == [b + 1 for b in before]
    for a, b in zip(blocks_of(out, env), blocks_of(base, env)):
        assert a.shape[0] == blocks and np.array_equal(a, b)
    assert (out.Scale, out.Dim, out.Format) == (base.Scale, base.Dim, base.Format)
    got = out.Decrypt(env)
    assert np.array_equal(got, base.Decrypt(env))
    if shift > 0:                                            # column c at slots c shift .. c shift + dim - 1; the result is registered with the columns' Dim
        assert np.array_equal(got[:dim], data[:, 0])
    m.Dispose()


def test_permute_returns_the_words_of_the_switch_off_run(fx, monkeypatch):
    from cryptonets_amd import hewrapper
    from cryptonets_amd.hewrapper import EVectorFormat
    F, env = fx
    values = np.arange(1, 11, dtype=float)
    v = F.GetEncryptedVector(values, EVectorFormat.dense, 1)
    sel = []
    for hot in ([1, 4], [3, 6], [0, 9]):
        s = np.zeros(10)
        s[hot] = 1.0
        sel.append(F.GetPlainVector(s, EVectorFormat.dense, 1))
    selections, shifts = [sel[0], None, sel[1], sel[2]], [1, 7, 3, 0]          # 3 = 4 - 1 in hops (default keys); 0: a plain addend
    before = summed(env)
    base = v.Permute(selections, shifts, 10, env)
    assert summed(env) == before
    monkeypatch.setattr(hewrapper, "SUMMED_ROTATIONS", True)
    out = v.Permute(selections, shifts, 10, env)
    assert summed(env) == [b + 1 for b in before]
    for a, b in zip(dh.words(out, env), dh.words(base, env)):
        assert np.array_equal(a, b)
    assert (out.Scale, out.Dim, out.Format) == (base.Scale, base.Dim, base.Format)
    # slot i of the result: values[i + 1] where selection 0 is hot, values[i + 3] where selection 2 is, values[i] where selection 3 is
    assert list(out.Decrypt(env)[:10]) == [2 + 4 + 1, 0, 0, 5 + 7, 0, 0, 0, 0, 0, 10]


@pytest.mark.parametrize("B, folding", [(256, True), (64, False)], ids=["folding", "gaps"])
def test_diagonal_dense_decrypts_to_the_product_in_both_plan_shapes(fx, monkeypatch, B, folding):
    from cryptonets_amd import hewrapper
    from cryptonets_amd.hewrapper import EMatrixFormat, EVectorFormat
    F, env = fx
    R, dim = 37, 700
    W, v = dh.weights(R, dim, R + dim), dh.vector(dim, R + dim)
    m = F.GetPlainMatrix(W.astype(float), EMatrixFormat.RowMajor, 1.0)
    ev = F.GetEncryptedVector(v.astype(float), EVectorFormat.dense, 1.0)
    before = summed(env)
    base = m.DiagonalDense(ev, env, B=B)
    assert summed(env) == before
    plan = m._diagonal_plan(0, env.Environments[0], B)[0]
    assert bool(plan.giants_by_folding) == folding and plan.classes == [0, 1] and plan.Gs == 512 // B
    monkeypatch.setattr(hewrapper, "SUMMED_ROTATIONS", True)
    out = m.DiagonalDense(ev, env, B=B)
    assert summed(env) == [b + 1 for b in before]
    want = np.zeros(dh.N, dtype=np.int64)
    want[:R] = W @ v
    for vec in (out, base):
        for t, s in zip(dh.PRIMES, all_slots(vec, env)):     # every one of the N slots, per plaintext prime: W v mod t, zero above row 37
            assert np.array_equal(s, want % t) and not s[R:].any()
    assert (out.Scale, out.Dim, out.Format) == (base.Scale, base.Dim, base.Format) and out.Dim == R
    if not folding:                                          # the gaps route rotates every group and adds: the summed call writes its words
        for a, b in zip(dh.words(out, env), dh.words(base, env)):
            assert np.array_equal(a, b)
    m.Dispose()


def test_the_count_rule_prices_the_summed_giant_steps(fx, monkeypatch):
    """one pair of inverse transforms per column class instead of one per giant step: 2 k saved per further group with j > 0"""
    from cryptonets_amd import diagonal, hewrapper
    from cryptonets_amd.hewrapper import EMatrixFormat, EVectorFormat
    F, env = fx
    W, v = dh.weights(37, 700, 9), dh.vector(700, 9)
    m = F.GetPlainMatrix(W.astype(float), EMatrixFormat.RowMajor, 1.0)
    ev = F.GetEncryptedVector(v.astype(float), EVectorFormat.dense, 1.0)
    off = m.DiagonalDenseCounts(ev, env)
    monkeypatch.setattr(hewrapper, "SUMMED_ROTATIONS", True)
    on = m.DiagonalDenseCounts(ev, env)
    far = diagonal.structural_diagonals(37, 700, dh.N).reshape(2, -1, off["B"]).any(axis=2)[:, 1:]
    k = len(dh.TINY_Q)
    assert on["B"] == off["B"] and on["default"] == off["default"]
    assert off["diagonal"] - on["diagonal"] == (int(far.sum()) - int(far.any(axis=1).sum())) * 2 * k
    m.Dispose()
