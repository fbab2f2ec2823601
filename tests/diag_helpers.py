"""Shared by tests/test_diagonal_plan.py and tests/test_gpu_diagonal_dense.py: a two-prime factory on the smallest register-radix ring (N = 1024, m = 512; the
coefficient moduli of conftest's "tiny" set), small signed integer matrices, and the exact integer model of a dense layer's output slots."""
import numpy as np

from oracle_backend import OracleHarness

N = 1024
PRIMES = (12289, 40961)                                              # 1 mod 2048, far above the largest |W v| of the shapes below (700 * 3 * 3)
TINY_Q = [0xffffee001, 0xffffc4001, 0x1ffffe0001]
SHAPES = [(37, 700), (600, 300), (512, 512)]                         # the input spans both slot rows / the output does / exactly one row each


class TinyHarness(OracleHarness):
    def default_coeff_modulus(self, n):
        assert n == N
        return list(TINY_Q)


def make_factory(backend):
    from cryptonets_amd.hewrapper import EncryptedSealBfvFactory
    h = TinyHarness(backend)
    return EncryptedSealBfvFactory(PRIMES, N, 10, 20, -1, client_factory=h.client_factory, context_factory=h, galois=True)


def weights(R, dim, seed):
    """small signed integers, no zero row (the batched row path refuses zero plaintexts)"""
    rng = np.random.default_rng(seed)
    W = rng.integers(-3, 4, size=(R, dim))
    W[:, 0] = np.where(W.any(axis=1), W[:, 0], 1)
    return W


def vector(dim, seed):
    return np.random.default_rng(seed + 1000).integers(-3, 4, size=dim)


def expected_slots(W, v, n=N):
    """W v in slots 0 .. R - 1, zero above"""
    out = np.zeros(n, dtype=np.int64)
    out[:W.shape[0]] = W @ v
    return out


def decrypted_slots(vec, env):
    """all N slots of a single-block result as centred integers (CRT over the primes), whatever its registered Dim"""
    vals = []
    for i, e in enumerate(env.Environments):
        a = vec.eVectors[i].encData
        ct = e.ctx.ct_download(a.buf.h, a.first, 1)[0]
        vals.append(np.asarray(e.ctx.o.decode(e.client.decrypt(ct)) if hasattr(e.ctx, "o") else e.client.o.decode(e.client.decrypt(ct)), dtype=object))
    M = 1
    for t in PRIMES:
        M *= t
    x = np.zeros(N, dtype=object)
    for t, r in zip(PRIMES, vals):
        Mi = M // t
        x = (x + r * (Mi * pow(Mi % t, -1, t))) % M
    return np.array([int(c) - M if 2 * int(c) > M else int(c) for c in x], dtype=np.int64)


def words(vec, env):
    return [e.ctx.ct_download(vec.eVectors[i].encData.buf.h, vec.eVectors[i].encData.first, 1)[0] for i, e in enumerate(env.Environments)]
