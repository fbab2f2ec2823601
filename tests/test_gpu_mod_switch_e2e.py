"""GPU, end to end through the wrapper: network outputs switched to the lowest level whose noise budget stays at least one bit (SEAL's integer
budget, CryptoTracker), decrypted there, written and read back at that level - against the exact integer models of the networks."""
import io

import numpy as np
import pytest

from cryptonets_amd import cryptonets_mnist as cm
from cryptonets_amd.cryptotracker import INT_MAX, CryptoTracker
from oracle_backend import make_factory

pytestmark = pytest.mark.gpu


def lowest_level(vec, env):
    """the lowest level whose budget (every ciphertext, every plaintext prime) is >= 1 bit, and the vector switched there"""
    best = None
    for limbs in range(env.Limbs - 1, 0, -1):
        sw = vec.ModSwitchTo(limbs, env)
        lenv = env.Level(limbs)
        CryptoTracker.MinBudgetSoFar = INT_MAX
        try:
            budget = CryptoTracker.TestVectorBudget(sw, lenv)
        except Exception as ex:                                  # CryptoTracker.cs:45-51: a budget of zero throws
            assert "budget is zero" in str(ex)
            budget = 0
        if budget < 1:
            sw.Dispose()
            break
        if best is not None:
            best[1].Dispose()
        best = (limbs, sw)
    assert best is not None, "no level below the first keeps a budget"
    return best


def test_cryptonets_mnist_outputs_at_the_lowest_level():
    from test_cryptonets_mnist import build_network, int_model_mod_p, synthetic_images, weights
    Factory = make_factory("gpu", primes=cm.PLAIN_PRIMES, n=cm.N, galois=False)
    env = Factory.AllocateComputationEnv()
    images = synthetic_images(64, seed=5)
    net, _ = build_network(Factory, images)
    net.PrepareNetwork()
    out = net.GetNext()
    L = cm.layer_tables(*weights())
    x_int = np.rint(images / 256.0 * 16.0).astype(np.int64)
    models = [int_model_mod_p(x_int, L, e.plainmodulusValue) for e in env.Environments]
    limbs, sw = lowest_level(out.GetColumn(0), env)
    assert limbs < env.Limbs
    for c in range(10):
        col = out.GetColumn(c)
        s = col.ModSwitchTo(limbs, env)
        lenv = env.Level(limbs)
        assert all(v.Limbs == limbs for v in s.eVectors)
        for i, e in enumerate(lenv.Environments):
            got = np.array(s.eVectors[i]._decrypt_ints(e), dtype=np.uint64)
            assert np.array_equal(got, models[i][:, c]), (c, e.plainmodulusValue)
        s.Dispose()
    sw.Dispose()
    out.Dispose()


def test_lola_mnist_logits_at_the_lowest_level_and_through_write_read():
    from test_lola import PRIMES, image, int_logits, lola
    from cryptonets_amd.serialization import read_vector, write_vector
    Factory = make_factory("gpu", primes=PRIMES, n=8192, galois=True)
    env = Factory.AllocateComputationEnv()
    img = image(6)
    net = lola(Factory, img)
    net.PrepareNetwork()
    out = net.GetNext()
    col = out.GetColumn(0)
    exp = int_logits(img)
    M = env.bigFactor
    exp = [((v % M) - M) if (v % M) * 2 > M else (v % M) for v in exp]
    assert [int(x) for x in col.DecryptFullPrecision(env)] == exp
    limbs, sw = lowest_level(col, env)
    lenv = env.Level(limbs)
    assert [int(x) for x in sw.DecryptFullPrecision(lenv)] == exp
    assert np.array_equal(sw.Decrypt(lenv), col.Decrypt(env))
    # a level vector refuses to meet a first-level one (SEAL's parameter-mismatch check)
    with pytest.raises(Exception, match="parameter mismatch"):
        sw.eVectors[0].Add(col.eVectors[0], lenv.Environments[0])
    # the wrapper's Write / Read at the level: written with the level's parms_id, read back through the FIRST level's environment
    buf = io.StringIO()
    write_vector(buf, sw, lenv)
    back = read_vector(io.StringIO(buf.getvalue()), env)
    assert all(v.Limbs == limbs for v in back.eVectors)
    assert [int(x) for x in back.DecryptFullPrecision(lenv)] == exp
    # ModSwitchToNext on the level vector drops one more prime (or the chain ends)
    if limbs > 1:
        nxt = back.ModSwitchToNext(lenv)
        assert all(v.Limbs == limbs - 1 for v in nxt.eVectors)
        nxt.Dispose()
    for v in (back, sw, out):
        v.Dispose()
