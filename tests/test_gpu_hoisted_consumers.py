"""hewrapper.HOISTED_ROTATIONS on the device: the copies of Duplicate and the baby steps of DiagonalDense through cn_rotate_rows_hoisted.  N = 1024, the two
plaintext primes of tests/diag_helpers.py, keygen / encrypt / decrypt on the device (the keys for a list of steps are the device client's).

Order of the module, as a deployment would go: a factory with the DEFAULT Galois keys records the steps under the switch (networks.rotation_steps: its contexts
lack the direct keys, take the present route and still report the direct baby steps); a second factory generates keys for exactly that list; on it, with the
switch on, Duplicate (count 4) and DiagonalDense (a 20 x 40 matrix with full-range weights, B = 8, both primes) decrypt to the values of the switch-off run and to
the integer model, and "ks_hoisted" has moved on the context of every prime.  The switch is set inside the tests only."""
import numpy as np
import pytest

import diag_helpers as dh

pytestmark = pytest.mark.gpu

R, DIM, B = 20, 40, 8
DUP_DIM, DUP_COUNT = 200, 4                                 # PackingShift 256: copies at 256, 512 (the other row: column swap, step 0) and 768 (column swap, -256)


class TinyContexts:
    """context_factory of the wrapper: library contexts on the coefficient moduli of diag_helpers"""

    def default_coeff_modulus(self, n):
        assert n == dh.N
        return list(dh.TINY_Q)

    def __call__(self, n, t, q, dbc, gdbc):
        from cryptonets_amd._native import Context
        return Context(n, t, q=q, dbc=dbc, gdbc=gdbc, device=0)


def factory(steps=None):
    from cryptonets_amd.hewrapper import EncryptedSealBfvFactory
    return EncryptedSealBfvFactory(dh.PRIMES, dh.N, 10, 20, -1, context_factory=TinyContexts(), client_seed=77, steps=steps)


def operands(F):
    from cryptonets_amd.hewrapper import EMatrixFormat, EVectorFormat
    rng = np.random.default_rng(5)
    W = rng.integers(-20000, 20001, size=(R, DIM))          # residues over the whole range of both primes; |W v| <= 40 x 20000 x 3, far below the product of the primes / 2
    W[0, :5] = [20000, -20000, 12288, -6145, 1]
    v = dh.vector(DIM, 5)
    d = rng.integers(-3, 4, size=DUP_DIM)
    return (W, v, d, F.GetPlainMatrix(W.astype(float), EMatrixFormat.RowMajor, 1.0), F.GetEncryptedVector(v.astype(float), EVectorFormat.dense, 1.0),
            F.GetEncryptedVector(d.astype(float), EVectorFormat.dense, 1.0))


class OneDenseLayerAndADuplicate:
    """the smallest thing networks.rotation_steps evaluates: a source of one record that runs the two consumers"""
    Source = None
    Factory = None

    def PrepareNetwork(self):
        pass

    def GetNext(self):
        env = self.Factory.AllocateComputationEnv()
        _, _, _, m, v, d = operands(self.Factory)
        m.DiagonalDense(v, env, B=B)
        d.Duplicate(DUP_COUNT, env)
        self.Factory.FreeComputationEnv(env)
        return m                                            # (rotation_steps disposes what it is handed)


@pytest.fixture(scope="module")
def steps():
    """what networks.rotation_steps reports under the switch on a factory with the default keys"""
    from cryptonets_amd import hewrapper, networks
    F = factory()
    old = hewrapper.HOISTED_ROTATIONS
    try:
        hewrapper.HOISTED_ROTATIONS = False
        off = networks.rotation_steps(OneDenseLayerAndADuplicate(), F)
        hewrapper.HOISTED_ROTATIONS = True
        on = networks.rotation_steps(OneDenseLayerAndADuplicate(), F)
    finally:
        hewrapper.HOISTED_ROTATIONS = old
    return off, on


def test_rotation_steps_lists_the_direct_baby_steps(steps):
    (off, off_cols), (on, on_cols) = steps
    # 20 x 40 at B = 8: every baby step 0 .. 7 is needed.  Switch off: by doubling, the steps 1, 2, 4; switch on: every direct step 1 .. 7 beside them
    assert {1, 2, 4} <= set(off) and not {3, 5, 6, 7} & set(off)
    assert set(range(1, B)) <= set(on) and set(off) <= set(on)
    assert -256 in on and on_cols and off_cols               # the copies of Duplicate: one direct step and the column swap, with or without the switch


def test_consumers_decrypt_to_the_switch_off_values_and_the_integer_model(steps, monkeypatch):
    from cryptonets_amd import hewrapper
    F = factory(steps=steps[1][0])
    env = F.AllocateComputationEnv()
    ctxs = [e.ctx for e in env.Environments]
    assert len(ctxs) == 2 and all(c.has_galois_key(c.galois_elt_from_step(s)) for c in ctxs for s in range(1, B))
    W, v, d, m, ev, ed = operands(F)
    before = [c.get_option("ks_hoisted") for c in ctxs]
    base_dense, base_dup = m.DiagonalDense(ev, env, B=B), ed.Duplicate(DUP_COUNT, env)
    assert [c.get_option("ks_hoisted") for c in ctxs] == before, "the switch is off: no hoisted call"
    monkeypatch.setattr(hewrapper, "HOISTED_ROTATIONS", True)
    dense, dup = m.DiagonalDense(ev, env, B=B), ed.Duplicate(DUP_COUNT, env)
    # one hoisted call for the baby steps, two for the copies (one per source row) - on the context of every prime
    assert [c.get_option("ks_hoisted") for c in ctxs] == [b + 3 for b in before]
    want = (W @ v).astype(float)
    assert np.array_equal(dense.Decrypt(env), want) and np.array_equal(base_dense.Decrypt(env), want)
    assert (dense.Scale, dense.Dim, dense.Format) == (base_dense.Scale, base_dense.Dim, base_dense.Format) and dense.Dim == R
    block = np.zeros(256)
    block[:DUP_DIM] = d
    assert np.array_equal(dup.Decrypt(env), np.tile(block, DUP_COUNT)) and np.array_equal(base_dup.Decrypt(env), np.tile(block, DUP_COUNT))
    # other ciphertext words than the present route's (the contract of tests/hoisted_model.py), the same values
    assert not any(np.array_equal(a, b) for a, b in zip(dh.words(dense, env), dh.words(base_dense, env)))
    m.Dispose()
    F.FreeComputationEnv(env)


def test_a_context_without_the_direct_keys_keeps_the_present_route(monkeypatch):
    """default keys: the baby steps 3, 5, 6, 7 have no key of their own - CN_ERR_NOKEY inside, the words of the switch-off run outside"""
    from cryptonets_amd import hewrapper
    F = factory()
    env = F.AllocateComputationEnv()
    W, v, d, m, ev, ed = operands(F)
    base = m.DiagonalDense(ev, env, B=B)
    monkeypatch.setattr(hewrapper, "HOISTED_ROTATIONS", True)
    before = [e.ctx.get_option("ks_hoisted") for e in env.Environments]
    out = m.DiagonalDense(ev, env, B=B)
    assert [e.ctx.get_option("ks_hoisted") for e in env.Environments] == before
    for a, b in zip(dh.words(out, env), dh.words(base, env)):
        assert np.array_equal(a, b)
    assert np.array_equal(out.Decrypt(env), (W @ v).astype(float))
    m.Dispose()
    F.FreeComputationEnv(env)


def test_only_a_missing_key_or_a_missing_kernel_falls_back_and_noted_steps_are_cleared(monkeypatch):
    """hewrapper._rotate_hoisted: CN_ERR_NOKEY and the planner's "no kernel here" refusals mean "take the present route"; any other refusal is the caller's error
    and is raised.  Steps are noted on the context only while it records, and switching the recording off clears them."""
    from cryptonets_amd import hewrapper
    from cryptonets_amd._native import CN_ERR_ARG, CnError
    F = factory()
    ctx = F.AllocateComputationEnv().Environments[0].ctx
    monkeypatch.setattr(hewrapper, "HOISTED_ROTATIONS", True)
    h = ctx.ct_alloc(4)
    assert hewrapper._rotate_hoisted(ctx, h, 0, [1, 2], h, [1, 2])                  # default keys hold 1 and 2
    assert not hewrapper._rotate_hoisted(ctx, h, 0, [1, 3], h, [1, 2])              # no key for 3 ...
    assert ctx.rotation_steps()[0] == []                                            # ... and nothing noted: the context does not record
    ctx.set_option("record_steps", 1)
    assert not hewrapper._rotate_hoisted(ctx, h, 0, [1, 0, 3], h, [1, 2, 3])
    assert ctx.rotation_steps()[0] == [1, 3]
    ctx.set_option("record_steps", 0)
    assert ctx.rotation_steps()[0] == []
    ctx.set_option("legacy_ntt", 1)                                                 # no register-radix kernels: the present route
    try:
        assert not hewrapper._rotate_hoisted(ctx, h, 0, [1, 2], h, [1, 2])
    finally:
        ctx.set_option("legacy_ntt", 0)
    for bad in (([1, 512], [1, 2]), ([1, 2], [1, 1]), ([1], [0])):                  # a step of N / 2, an output listed twice, the input as output: raised
        with pytest.raises(CnError) as e:
            hewrapper._rotate_hoisted(ctx, h, 0, bad[0], h, bad[1])
        assert e.value.code == CN_ERR_ARG
    ctx.free(h)


def test_diagonal_counts_price_hoisting_only_where_the_keys_are_held(steps, monkeypatch):
    from cryptonets_amd import hewrapper
    counts = []
    for F in (factory(), factory(steps=steps[1][0])):                               # default keys; keys for the direct steps
        env = F.AllocateComputationEnv()
        _, _, _, m, ev, _ = operands(F)
        off = m.DiagonalDenseCounts(ev, env)
        monkeypatch.setattr(hewrapper, "HOISTED_ROTATIONS", True)
        on = m.DiagonalDenseCounts(ev, env)
        monkeypatch.setattr(hewrapper, "HOISTED_ROTATIONS", False)
        counts.append((off, on))
        m.Dispose()
    (off0, on0), (off1, on1) = counts
    B_ = off1["B"]
    if all(s in steps[1][0] for s in range(1, B_)):                                 # the second factory holds the baby steps of the B the count rule picks
        assert on1["diagonal"] < off1["diagonal"]
    assert on0 == off0 or off0["B"] <= 2                                             # default keys lack 3, 5, 6, ..: priced by doubling, as the run will go
